"""Missions inside a rollout -- a queue of re-plan records per stream, each fired by a tick number, by the goal of the leg the stream is on or by a lost
plan -- as device code compiled for the CPU (csrc/bmpc_rollout_kernel.inl with QU; tests/emu/bmpc_emu_rollout.cpp, once for one wave per stream and
once for teams of four under wave orders 0 and 1).  Everything is bit for bit against the contract's loop for one stream, emu_rollout.contract_loop with a queue:
{fused tick's text, tube text, log text, disturb text, splice + update text of the head record when it is due}.  B = 3 streams of emu_rollout.small_stream
behind a solved-out tick 0, T <= 10; one case at (1, 2), one at (10, 4) with T = 3."""
import inspect

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er, emu_stream_update as eup

SS, RP, ROLL = bstream.SS, bstream.RP, bstream.ROLL
H = er.H
BUILDS = [(1, 0), (4, 0), (4, 1)]      # (waves per stream, order of the waves in a wide phase)
_copy = er.copy_arrays


def _forth(args):
    """the arguments of replan_record of emu_rollout.leg_back with the via points in the stream's own order again: a leg forth"""
    a = list(args)
    for i in (0, 1, 6, 7, 8, 9, 10):
        a[i] = a[i][::-1]
    for i in (2, 3):
        a[i] = [a[i][0][::-1], a[i][1][::-1]]
    return a


def _records(N, S, forth=False, **leg):
    """[B][len]: a leg back (or forth) per stream of the small batch"""
    streams = [er.small_stream(N, S, which=b) for b in range(3)]
    cap = streams[0][2].shape[0]
    make = lambda m, rec, Tb: _forth(er.leg_back(m, rec, Tb, S, **leg)) if forth else er.leg_back(m, rec, Tb, S, **leg)
    return np.ascontiguousarray(np.stack([bstream.replan_record(S, cap, *make(m, rec, Tb)) for m, rec, Tb, _ in streams]))


def _queue(N, S, K):
    """[B][K][len]: legs back, forth, back (with a detour), ... per stream"""
    kinds = [_records(N, S), _records(N, S, forth=True), _records(N, S, detour=0.05)]
    return np.ascontiguousarray(np.stack([kinds[k % 3] for k in range(K)], axis=1))


def _words(B, K, tick=-1, on=0):
    return np.full((B, K), tick, dtype=np.int32), np.full((B, K), on, dtype=np.int32)


# ---- (a) the degenerate cases ----
@pytest.mark.parametrize("nw,wave_order", BUILDS)
def test_one_tick_triggered_record_is_the_log_entry(nw, wave_order):
    """legs = 1, leg_on = 0, leg_tick = replan_tick against the existing level with everything (3) on the same inputs: every tick array, table, record and
    output; with every queue pointer NULL against that level without a re-plan (the level that runs there IS 3)"""
    N, S, T = 2, 2, 6
    A0, Tab, recs = er.start(N, S, nw)
    tick_of = np.array([2, -1, T - 1])
    dist = er.disturbances(T, 3, on=(1, 4))
    A, Tb, R = _copy(A0), Tab.copy(), recs.copy()
    want = er.rollout(N, S, H, Tb, A, T, nw=nw, wave_order=wave_order, entry=3, replan=R, replan_tick=tick_of, disturb=dist, log_stages=N)
    C, Tc, Rc = _copy(A0), Tab.copy(), recs[:, None].copy()
    r = er.rollout(N, S, H, Tc, C, T, entry=4, nw=nw, wave_order=wave_order, replan=Rc, leg_tick=tick_of[:, None], leg_on=np.zeros((3, 1)), disturb=dist, log_stages=N)
    assert want["ran"] == 3 and r["ran"] == 4
    for k in er.TICK_ARRAYS:
        assert np.array_equal(A[k], C[k], equal_nan=True), k
    assert np.array_equal(Tb, Tc) and np.array_equal(R, Rc[:, 0]) and not np.array_equal(Tb, Tab)
    for k in ("hist", "traj_hist", "ticks_run", "tube_hist", "audit", "log_hist", "track"):
        assert np.array_equal(want[k], r[k], equal_nan=True), k
    assert np.array_equal(want["replan_info"], r["replan_info"][:, 0]) and r["replan_info"][:, 0].tolist() == [0, -1, 0]
    assert r["legs_done"].tolist() == [1, 0, 1] and r["leg_fired"][:, 0].tolist() == [2, -1, T - 1] and r["leg_why"][:, 0].tolist() == [er.WHY_TICK, 0, er.WHY_TICK]
    # without records: the log entry without a re-plan, and the queue arguments are not looked at (legs = 0 among them)
    A, Tb = _copy(A0), Tab.copy()
    want = er.rollout(N, S, H, Tb, A, T, nw=nw, wave_order=wave_order, entry=3, disturb=dist, log_stages=N)
    C, Tc = _copy(A0), Tab.copy()
    r = er.rollout(N, S, H, Tc, C, T, entry=4, nw=nw, wave_order=wave_order, legs=0, want_done=False, want_fired=False, disturb=dist, log_stages=N)
    assert r["ran"] == want["ran"] == 3 and np.array_equal(Tc, Tab)
    for k in er.TICK_ARRAYS:
        assert np.array_equal(A[k], C[k], equal_nan=True), k
    for k in ("hist", "traj_hist", "ticks_run", "tube_hist", "audit", "log_hist", "track"):
        assert np.array_equal(want[k], r[k], equal_nan=True), k


# ---- (b) ticks ----
def _tick_case(N, S, nw=1):
    """stream 0: records at ticks 1, 3, 5; stream 1: three records all at tick 2 (they fire behind 2, 3 and 4); stream 2: an end-of-queue word (an
    unknown bit, with a tick condition that would hold) at the head of records that would be due"""
    A0, Tab, _ = er.start(N, S, nw)
    Q = _queue(N, S, 3)
    lt = np.array([[1, 3, 5], [2, 2, 2], [0, 1, 2]], dtype=np.int32)
    lo = np.array([[0, 0, 0], [0, 0, 0], [4, 0, 0]], dtype=np.int32)
    return A0, Tab, Q, lt, lo


@pytest.mark.parametrize("nw,wave_order", BUILDS)
def test_records_scheduled_by_tick_fire_in_queue_order(nw, wave_order):
    N, S, T = 2, 2, 8
    A0, Tab, Q, lt, lo = _tick_case(N, S, nw)
    dist = er.disturbances(T, 3, on=(1, 4))
    r, A, Tb, R, _ = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"ticks, nw {nw} order {wave_order}", leg_tick=lt, leg_on=lo, leg_tol=None, nw=nw, wave_order=wave_order, stages=N, disturb=dist)
    assert r["ticks_run"].tolist() == [T] * 3 and r["legs_done"].tolist() == [3, 3, 0]
    assert r["leg_fired"].tolist() == [[1, 3, 5], [2, 3, 4], [-1, -1, -1]] and r["leg_why"].tolist() == [[4, 4, 4], [4, 4, 4], [0, 0, 0]]
    assert r["replan_info"].tolist() == [[0, 0, 0], [0, 0, 0], [-1, -1, -1]]
    assert (R[:2, :, RP["FLAG"]] == 0).all() and np.array_equal(R[2], Q[2]) and np.array_equal(Tb[2], Tab[2]) and not np.array_equal(Tb[0], Tab[0])
    # every re-plan took: phi starts again on a new first segment behind each fired tick
    phi = r["hist"][:, 0, ROLL["PHI"]]
    assert all(phi[t + 1] < phi[t] for t in (1, 3, 5))
    # the audit and the tracking record run over the whole mission
    assert r["audit"][:, bstream.AUDIT["SAMPLES"]].tolist() == [T] * 3 and (r["track"][:, bstream.TRACK["SAMPLES"]] == T).all()


@pytest.mark.parametrize("N,S,T", [(1, 2, 6), (10, 4, 3)])
def test_other_shapes(N, S, T):
    """the smallest horizon and the reference's shape: a record behind ticks 0 and 1 of stream 0, a goal record whose tolerance is the whole path (due at
    once) ahead of a tick record for stream 1, an empty word for stream 2"""
    A0, Tab, _ = er.start(N, S)
    Q = _queue(N, S, 2)
    lt = np.array([[0, 1], [-1, T - 1], [-1, -1]], dtype=np.int32)
    lo = np.array([[0, 0], [er.AT_GOAL, 0], [0, 0]], dtype=np.int32)
    tol = np.full((3, 2), 100.0)
    r, _, _, R, _ = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"N {N} S {S}", leg_tick=lt, leg_on=lo, leg_tol=tol, stages=N)
    assert r["legs_done"].tolist() == [2, 2, 0] and r["leg_fired"].tolist() == [[0, 1], [0, T - 1], [-1, -1]]
    assert r["leg_why"].tolist() == [[4, 4], [er.WHY_GOAL, er.WHY_TICK], [0, 0]] and np.array_equal(R[2], Q[2])


# ---- (c) goals ----
def _goal_case(N, S, T, nw=1):
    """Two goal-triggered legs per stream, back and forth.  The goals are far away (phi_max 6.2 to 6.9, phi of the order 1e-3 behind a few ticks), so
    record k of stream b gets the tolerance phi_max - c with c between two values of the stream's own phi trace: it fires on a chosen tick.  The traces
    come from probes of the loop: without records (leg 1), with the first record (leg 2), with both (leg 3: the last goal and goal_tol).
    -> (A0, Tab, Q, leg_tick, leg_on, leg_tol, goal_tol, the ticks chosen [B][2], the stop tick chosen for stream 1)"""
    A0, Tab, _ = er.start(N, S, nw)
    Q = _queue(N, S, 2)
    lt, lo = _words(3, 2, on=er.AT_GOAL)
    tol = np.zeros((3, 2))
    at = np.array([[1, 4], [2, 4], [3, 6]])      # the ticks behind which the records shall fire
    probe = lambda b, K, goal_tol=0.0: er.contract_loop(N, S, H, Tab[b].copy(), er.unstack(A0, b), T, replan=Q[b, :K].copy(), leg_tick=lt[b], leg_on=lo[b], leg_tol=tol[b],
                                                       goal_tol=goal_tol, nw=nw)
    for b in range(3):
        for k in range(2):
            tr = probe(b, k)
            t = at[b, k]
            fresh = k > 0 and at[b, k - 1] == t - 1      # (the first tick of a leg: nothing of this leg ahead of it)
            lo_phi = 0.0 if fresh else tr["phi"][t - 1]
            assert tr["phi"][t] > lo_phi and tr["phi_max"][t] == tr["phi_max"][T - 1]
            tol[b, k] = tr["phi_max"][t] - 0.5 * (lo_phi + tr["phi"][t])
    # the last goal: stream 1 stops behind tick 6 of T = 9 -- streams 0 and 2 have longer paths and the same tolerance does not reach them
    tr, stop = probe(1, 2), 6
    goal_tol = float(tr["phi_max"][stop] - 0.5 * (tr["phi"][stop - 1] + tr["phi"][stop]))
    return A0, Tab, Q, lt, lo, tol, goal_tol, at, stop


@pytest.mark.parametrize("nw,wave_order", BUILDS)
def test_goal_triggered_legs_follow_each_other_at_every_streams_own_pace(nw, wave_order):
    N, S, T = 2, 2, 9
    A0, Tab, Q, lt, lo, tol, goal_tol, at, stop = _goal_case(N, S, T, nw)
    r, A, Tb, R, _ = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"goals, nw {nw} order {wave_order}", leg_tick=lt, leg_on=lo, leg_tol=tol, nw=nw, wave_order=wave_order, goal_tol=goal_tol)
    print("fired", r["leg_fired"].tolist(), "why", r["leg_why"].tolist(), "ticks_run", r["ticks_run"].tolist(), "leg_tol", tol.tolist(), "goal_tol", goal_tol)
    two = [b for b in range(3) if r["legs_done"][b] == 2]
    assert len(two) >= 2                                                                   # at least two streams consumed two records each
    assert all(r["leg_why"][b].tolist() == [er.WHY_GOAL, er.WHY_GOAL] for b in two)        # by the goal alone
    assert len({tuple(r["leg_fired"][b]) for b in two}) >= 2                               # each at its own ticks
    short = [b for b in range(3) if r["ticks_run"][b] < T]
    assert short and all(np.isnan(r["hist"][r["ticks_run"][b]:, b]).all() and np.isfinite(r["hist"][:r["ticks_run"][b], b]).all() for b in short)
    # ... and exactly as constructed
    assert r["leg_fired"].tolist() == at.tolist() and r["ticks_run"].tolist() == [T, stop + 1, T] and (r["replan_info"] == 0).all()
    # with goal_tol > 0 a stream stops only at the goal of its LAST leg: the same launch without the queue stops stream 1 no later (its first goal is nearer)
    assert (R[:, :, RP["FLAG"]] == 0).all() and (A["ss"][:, SS["PHIMAX"]] != A0["ss"][:, SS["PHIMAX"]]).all()


# ---- (d) rescue ----
def _rescue_case(N, S, nw=1):
    """the rescue scenario of tests/test_stream_rollout_events.py: tick 0 solved out, then plants a push has carried 16 cm off their paths (tube half
    width 1 cm) under one-iteration ticks: every tick fails, from error count 0 a stream runs N = 2 ticks and is lost.  Stream 0 holds an ON_LOST
    record, stream 1 an empty word, stream 2 is lost on entry (it never runs a tick, so its ON_LOST record is never looked at)."""
    A0, Tab, _ = er.start(N, S, nw)
    A0 = _copy(A0)
    push = np.zeros(21); push[:4] = [0.1, -0.1, 0.1, 0.1]
    for b in range(3):
        A0["rb"][b] = eup.stream_disturb(A0["rb"][b], push)
    A0["ss"][2, SS["ERRCNT"]] = N
    Q = _queue(N, S, 2)
    lt, lo = _words(3, 2)
    lo[0, 0] = lo[2, 0] = er.ON_LOST
    return A0, Tab, Q, lt, lo


@pytest.mark.parametrize("nw,wave_order", BUILDS)
def test_an_on_lost_record_rescues_the_stream(nw, wave_order):
    N, S, T = 2, 2, 6
    A0, Tab, Q, lt, lo = _rescue_case(N, S, nw)
    r, A, Tb, R, _ = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"rescue, nw {nw} order {wave_order}", leg_tick=lt, leg_on=lo, leg_tol=None, nw=nw, wave_order=wave_order, max_iter=1)
    off = er.rollout(N, S, H, Tab.copy(), _copy(A0), T, entry=4, nw=nw, wave_order=wave_order, replan=Q.copy(), leg_tick=lt, leg_on=np.zeros_like(lo), max_iter=1)
    assert off["ticks_run"].tolist() == [2, 2, 0] and off["legs_done"].tolist() == [0, 0, 0]
    # the record fires behind the post that exhausted the plan, with WHY lost, and the stream runs on where the launch without it stops
    assert r["leg_fired"].tolist() == [[1, -1], [-1, -1], [-1, -1]] and r["leg_why"].tolist() == [[er.WHY_LOST, 0], [0, 0], [0, 0]] and r["legs_done"].tolist() == [1, 0, 0]
    assert r["ticks_run"][0] > 2 and r["ticks_run"].tolist()[1:] == [2, 0] and r["hist"][1, 0, ROLL["ERRCNT"]] == N
    assert R[:, :, RP["FLAG"]].tolist() == [[0.0, 1.0], [1.0, 1.0], [1.0, 1.0]] and np.array_equal(Tb[1:], Tab[1:])
    # solved to tolerance the rescue is one in earnest: the new path starts where the plant is, and the stream runs every tick
    full = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, "rescue, solved to tolerance", leg_tick=lt, leg_on=lo, leg_tol=None, nw=nw, wave_order=wave_order)[0]
    assert full["ticks_run"].tolist() == [T, 2, 0] and full["leg_fired"][0, 0] == 1 and (full["hist"][2:, 0, ROLL["SUCCESS"]] == 1).all()


# ---- (e) mixed conditions, records that do nothing, records never reached ----
@pytest.mark.parametrize("nw,wave_order", BUILDS)
def test_mixed_conditions_and_records_that_are_consumed_without_effect(nw, wave_order):
    """Record 0 of every stream: goal or tick 3, whichever first -- stream 0's goal tolerance is met behind tick 1 (goal alone), stream 1's never (tick
    alone), stream 2's behind tick 3 (both).  Record 1, at tick 4: lowered flag (stream 0), invalid (stream 1: n = 1), fine (stream 2).  Record 2: at tick
    5 (streams 0, 1), at tick 100 (stream 2: never reached, keeps its flag)."""
    N, S, T = 2, 2, 7
    A0, Tab, _ = er.start(N, S, nw)
    Q = _queue(N, S, 3)
    Q[0, 1, RP["FLAG"]] = 0.0
    Q[1, 1, RP["N"]] = 1.0
    lt = np.array([[3, 4, 5], [3, 4, 5], [3, 4, 100]], dtype=np.int32)
    lo = np.array([[1, 0, 0], [1, 0, 0], [1, 0, 0]], dtype=np.int32)
    tol = np.zeros((3, 3))
    for b, t in ((0, 1), (2, 3)):
        tr = er.contract_loop(N, S, H, Tab[b].copy(), er.unstack(A0, b), T, nw=nw)
        tol[b, 0] = tr["phi_max"][t] - 0.5 * (tr["phi"][t - 1] + tr["phi"][t])
    r, A, Tb, R, _ = er.assert_equals_the_loop(N, S, A0, Tab, Q, T, f"mixed, nw {nw} order {wave_order}", leg_tick=lt, leg_on=lo, leg_tol=tol, nw=nw, wave_order=wave_order)
    assert r["leg_fired"].tolist() == [[1, 4, 5], [3, 4, 5], [3, 4, -1]] and r["legs_done"].tolist() == [3, 3, 2]
    assert r["leg_why"].tolist() == [[er.WHY_GOAL, 4, 4], [er.WHY_TICK, 4, 4], [er.WHY_GOAL | er.WHY_TICK, 4, 0]]
    assert r["replan_info"].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, -1]]
    # the lowered record is untouched, the invalid one has only its flag cleared, the record never reached keeps its flag
    assert np.array_equal(R[0, 1], Q[0, 1]) and R[1, 1, RP["FLAG"]] == 0.0 and np.array_equal(R[1, 1, 1:], Q[1, 1, 1:]) and np.array_equal(R[2, 2], Q[2, 2])
    # ... and neither touched its stream: the rows behind tick 4 are those of the mission without that record's turn
    S0 = er.rollout(N, S, H, Tab.copy(), _copy(A0), T, entry=4, nw=nw, wave_order=wave_order, replan=Q[:, [0, 2]].copy(), leg_tick=lt[:, [0, 2]], leg_on=lo[:, [0, 2]],
                         leg_tol=tol[:, [0, 2]])
    assert np.array_equal(S0["hist"][:, :2], r["hist"][:, :2])


# ---- (f) the refusals ----
def test_argument_errors_of_the_entry():
    N, S = 2, 2
    A0, Tab, _ = er.start(N, S)
    Q = _queue(N, S, 2)
    lt, lo = _words(3, 2, tick=1)
    ok = dict(replan=Q, leg_tick=lt, leg_on=lo)
    bad = [dict(ok, leg_tick=None), dict(ok, leg_on=None), dict(ok, want_done=False), dict(ok, legs=0), dict(ok, legs=-1),
           dict(ok, update_flags=8), dict(ok, update_flags=4), dict(update_flags=16), dict(ok, ticks=0), dict(ok, simulate=False), dict(ok, goal_tol=-1.0), dict(ok, goal_tol=np.nan),
           dict(ok, audit_tol=-1.0), dict(ok, audit_tol=np.inf), dict(ok, log_stages=0), dict(ok, log_stages=N + 1), dict(audit_tol=np.nan), dict(log_stages=0)]
    for kw in bad:
        A, Tb = _copy(A0), Tab.copy()
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else Q.copy()
        assert er.rollout(N, S, H, Tb, A, kw.pop("ticks", 2), entry=4, want_rc=True, **kw) == 1, {k: v for k, v in kw.items() if k != "replan"}
        for b in range(3):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
        assert np.array_equal(Tb, Tab) and (kw["replan"] is None or np.array_equal(kw["replan"], Q))
    # allowed: the per-record outputs and tolerances NULL, no records with any queue argument, log_stages not looked at without the log's arrays
    for kw in (dict(ok, want_fired=False), dict(legs=-5, want_done=False), dict(ok, log_stages=0, want_log=False, track=False)):
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else Q.copy()
        assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=4, want_rc=True, **kw) == 0
    # the trigger words are not validated: negative words, huge ticks and unknown bits run and end the queue
    lo2 = np.array([[-1, 0], [8, 0], [1 << 30, 0]], dtype=np.int32)
    r = er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=4, replan=Q.copy(), leg_tick=np.zeros((3, 2)), leg_on=lo2)
    assert r["legs_done"].tolist() == [0, 0, 0] and (r["leg_fired"] == -1).all()


def test_the_python_surface():
    L = bstream.LEG
    assert (L["AT_GOAL"], L["ON_LOST"], L["WHY_GOAL"], L["WHY_LOST"], L["WHY_TICK"]) == (er.AT_GOAL, er.ON_LOST, er.WHY_GOAL, er.WHY_LOST, er.WHY_TICK) == (1, 2, 1, 2, 4)
    assert {"legs", "leg_tick", "leg_on", "leg_tol"} <= set(inspect.signature(bstream.StreamBatch.rollout).parameters)
    from boundmpc_amd import _lib
    assert len(_lib.SIGNATURES["bmpc_stream_rollout_legs"][1]) == len(_lib.SIGNATURES["bmpc_stream_rollout_log"][1]) - 1 + 7


# ---- (g) the stand-alone program under the sanitizers ----
def sanitizer_cases(nw):
    """cases (b) to (d) as case files of the stand-alone program"""
    N, S = 2, 2
    A0, Tab, Q, lt, lo = _tick_case(N, S, nw)
    cases = [("ticks", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=8, recs=Q, leg_tick=lt, leg_on=lo, disturb=er.disturbances(8, 3, on=(1, 4))))]
    A0, Tab, Q, lt, lo, tol, goal_tol, _, _ = _goal_case(N, S, 9, nw)
    cases.append(("goals", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=9, recs=Q, leg_tick=lt, leg_on=lo, leg_tol=tol, goal_tol=goal_tol)))
    A0, Tab, Q, lt, lo = _rescue_case(N, S, nw)
    cases.append(("rescue", dict(N=N, S=S, h=H, T=Tab, A=A0, ticks=6, recs=Q, leg_tick=lt, leg_on=lo, max_iter=1)))
    return cases


@pytest.mark.parametrize("nw", [1, 4])
def test_the_queue_text_is_clean_under_the_sanitizers(nw):
    """the host program with its own main, built with -fsanitize=address,undefined on exact-size buffers and run as a child process (nothing is loaded
    into this interpreter): cases (b) to (d), on teams under both wave orders; what it prints agrees with this module's expectations"""
    out = er.run_sanitized(sanitizer_cases(nw), nw)
    print("\n".join(out))
    assert len(out) == 3 and all("rc 0 ran 4" in line and "DIFFERS" not in line for line in out)
    assert "[stream 0 ticks_run 8 legs_done 3 fired 1 3 5 why 4 4 4 info 0 0 0]" in out[0] and "[stream 1 ticks_run 8 legs_done 3 fired 2 3 4" in out[0]
    assert "[stream 2 ticks_run 8 legs_done 0 fired -1 -1 -1 why 0 0 0 info -1 -1 -1]" in out[0]
    assert "[stream 1 ticks_run 7 legs_done 2 fired 2 4 why 1 1 info 0 0]" in out[1]
    assert "legs_done 1 fired 1 -1 why 2 0 info 0 -1]" in out[2] and "[stream 2 ticks_run 0 legs_done 0" in out[2]
