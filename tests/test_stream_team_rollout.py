"""CPU: the TEAM rollout -- csrc/bmpc_rollout_kernel.inl compiled with BMPC_NW = 4 waves per stream (namespace bmpct), both instantiations of
csrc/bmpc_team_rollout.hip, as a g++ build of their own text (tests/emu/bmpc_emu_rollout.cpp with -DBMPC_NW=4) -- against its exact checker: a loop of the team
tick's own kernel text (emu.stream_tick(nw=4)) and, for the fully-featured kernel, the loop {team tick, tube, log rows, disturb, update} assembled from the
existing emulator functions.  Bit for bit where the same text runs (tick arrays, history, tube and log rows, tables, records); the audit and tracking
records against their numpy specifications within 1e-11, their integer slots exactly.  Under wave orders 0 (forward) and 1 (reverse): a wide phase of
the team is a loop over its waves here, and the result must not depend on their order.
What a CPU build cannot show is a team whose waves disagree at a barrier (one thread runs all waves here); that is argued in the kernel text: every
exit of the tick loop is decided by every wave from ss, r.replan_tick and kernel arguments, read behind the barrier that follows their last store."""
import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu_rollout as er, emu_stream_tube as et

ROLL, SS, TRACK, AUDIT = bstream.ROLL, bstream.SS, bstream.TRACK, bstream.AUDIT
H, NW = 0.1, 4


def _one(A0):
    """the tick arrays of one stream as a batch of one"""
    return er.stack([A0])


def _assert_batch_equals(batch, b, A, what):
    for k in er.TICK_ARRAYS:
        assert np.array_equal(np.ravel(batch[k][b]), np.ravel(A[k]), equal_nan=True), f"{what}: {k} differs"


def _compare_plain(N, S, T, A0, ticks, wave_order, what, **kw):
    """the plain team rollout on a copy of A0 against `ticks` team ticks on another, under one wave order for both"""
    loop = er.copy_arrays(A0)
    want = er.contract_loop(N, S, H, T, loop, ticks, nw=NW, wave_order=wave_order, **kw)
    rows, trajs, snaps = want["hist"], want["traj_hist"], want["snaps"]
    batch = _one(A0)
    r = er.rollout(N, S, H, np.ascontiguousarray(T[None]), batch, ticks, nw=NW, wave_order=wave_order, **kw)
    assert r["ticks_run"][0] >= 1, what
    _assert_batch_equals(batch, 0, loop, what)
    assert r["ticks_run"][0] == int(np.isfinite(rows[:, ROLL["STATUS"]]).sum()), what
    assert np.array_equal(r["hist"][:, 0], rows, equal_nan=True) and np.array_equal(r["traj_hist"][:, 0], trajs, equal_nan=True), what
    return r, batch, rows, snaps


@pytest.mark.parametrize("wave_order", [0, 1])
@pytest.mark.parametrize("N,S", [(2, 2), (1, 2)])
def test_team_rollout_equals_the_team_tick_loop_bit_for_bit(N, S, wave_order):
    """T = 4 converged ticks with the dual state carried, from the cold start; every tick runs, and the plant moves"""
    _, rec, T, ss = er.small_stream(N, S)
    r, batch, rows, _ = _compare_plain(N, S, T, er.fresh_arrays(N, S, ss, rec), 4, wave_order, f"N {N} S {S} wave order {wave_order}", warm_dual=True)
    assert r["ticks_run"][0] == 4 and np.isfinite(r["hist"]).all() and (r["hist"][:, 0, ROLL["STATUS"]] == 0).all()
    assert (np.diff(r["hist"][:, 0, ROLL["PHI"]]) > 0).all()
    if wave_order:      # ... and the same bits as under the forward order
        other = _one(er.fresh_arrays(N, S, ss, rec))
        r0 = er.rollout(N, S, H, np.ascontiguousarray(T[None]), other, 4, nw=NW, warm_dual=True)
        assert np.array_equal(r0["hist"], r["hist"])
        _assert_batch_equals(batch, 0, er.unstack(other, 0), "wave order 1 against 0")


@pytest.mark.parametrize("wave_order", [0, 1])
def test_a_stream_that_loses_its_plan_stops(wave_order):
    """(10, 4): tick 0 solved out, then two iterations per tick without the real-time rule (the case of tests/test_stream_rollout.py): the error count
    climbs to N, status 3 is written once, the rows behind are NaN; lost on entry: no tick"""
    N, S, ticks = 10, 4, 13
    _, rec, T, ss = er.small_stream(N, S)
    A0 = er.fresh_arrays(N, S, ss, rec)
    er.tick(N, S, H, T, A0, max_iter=100, warm_dual=True, nw=NW, wave_order=wave_order)
    assert A0["status"][0] == 0 and A0["ss"][SS["ERRCNT"]] == 0
    r, batch, rows, snaps = _compare_plain(N, S, T, A0, ticks, wave_order, f"lost plan, wave order {wave_order}", max_iter=2, warm_dual=True)
    ec = rows[:, ROLL["ERRCNT"]]
    implied = int(np.argmax(ec >= N)) + 1
    assert (ec >= N).any() and 1 <= implied < ticks and r["ticks_run"][0] == implied
    assert np.isnan(r["hist"][implied:]).all() and np.isnan(r["traj_hist"][implied:]).all() and np.isfinite(r["hist"][:implied]).all()
    B = er.unstack(batch, 0)
    assert B["status"][0] == 3 and B["iters"][0] == 0 and B["kkt"][0] == 0.0 and B["ss"][SS["ERRCNT"]] == N
    keep = er.copy_arrays(snaps[implied - 1]); keep["status"][0], keep["iters"][0], keep["kkt"][0] = 3, 0, 0.0
    er.assert_arrays_equal(keep, B, "behind the stop")
    C = _one(B); C["status"][0], C["iters"][0], C["kkt"][0] = 7, 7, 7.0
    r2 = er.rollout(N, S, H, np.ascontiguousarray(T[None]), C, 3, nw=NW, max_iter=2, warm_dual=True, wave_order=wave_order)
    assert r2["ticks_run"][0] == 0 and np.isnan(r2["hist"]).all() and np.isnan(r2["traj_hist"]).all()
    _assert_batch_equals(C, 0, B, "lost on entry")


# ---- the fully-featured kernel: (2, 2), B = 3, T = 6 ----
N, S, T = 2, 2, 6
TOL = 1e-6
REPLAN_TICK = np.array([-1, -1, 3])


_copy = er.copy_arrays


@pytest.mark.parametrize("wave_order", [0, 1])
def test_full_kernel_without_events_equals_the_plain_kernel(wave_order):
    """every event, audit and log pointer NULL: the arrays, the history and ticks_run of the plain team rollout, bit for bit"""
    A0, Tab, _ = er.start(N, S, NW)
    P, F = _copy(A0), _copy(A0)
    plain = er.rollout(N, S, H, Tab.copy(), P, T, nw=NW, opts=er.opts(N), wave_order=wave_order)
    full = er.rollout(N, S, H, Tab.copy(), F, T, nw=NW, entry=1, opts=er.opts(N), wave_order=wave_order)      # (level 1: the teams run the kernel with everything)
    assert plain["ticks_run"].tolist() == [T] * 3 and full["replan_info"].tolist() == [-1] * 3 and (plain["ran"], full["ran"]) == (0, 3)
    for k in er.TICK_ARRAYS:
        assert np.array_equal(P[k], F[k], equal_nan=True), k
    for k in ("hist", "traj_hist", "ticks_run"):
        assert np.array_equal(plain[k], full[k], equal_nan=True), k
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), T, nw=NW, opts=er.opts(N), audit=True, want_rc=True) == 1      # (the plain kernel takes no such array)


@pytest.mark.parametrize("wave_order", [0, 1])
def test_full_kernel_with_everything_raised_equals_the_assembled_loop(wave_order):
    """a disturbance behind tick 2 of stream 1, a re-plan with splice behind tick 3 of stream 2, audit, tube rows, log rows of two stages and the
    tracking record, against the loop {team tick, tube, log rows, disturb, update} per stream"""
    A0, Tab, recs = er.start(N, S, NW)
    d = er.push(T, 3)
    A, Tb, R = _copy(A0), Tab.copy(), recs.copy()
    r = er.rollout(N, S, H, Tb, A, T, nw=NW, entry=3, replan=R, replan_tick=REPLAN_TICK, update_flags=3, disturb=d, opts=er.opts(N), wave_order=wave_order, audit=True, want_tube=True,
                    audit_tol=TOL, want_log=True, log_stages=2, track=True)
    assert r["ticks_run"].tolist() == [T] * 3 and r["replan_info"].tolist() == [-1, -1, 0]
    for b in range(3):
        Ab, Tl, Rl = er.unstack(A0, b), Tab[b].copy(), recs[b].copy()
        want = er.contract_loop(N, S, H, Tl, Ab, T, stages=2, replan=Rl, replan_tick=int(REPLAN_TICK[b]), update_flags=3, disturb=d[:, b], opts=er.opts(N), nw=NW, wave_order=wave_order)
        _assert_batch_equals(A, b, Ab, f"stream {b}")
        assert np.array_equal(Tb[b], Tl) and np.array_equal(R[b], Rl), b
        for k in ("hist", "traj_hist", "tube_hist", "log_hist"):
            assert np.array_equal(r[k][:, b], want[k], equal_nan=True), (b, k)
        assert r["ticks_run"][b] == want["ticks_run"] and r["replan_info"][b] == want["replan_info"]
    assert not np.array_equal(Tb[2], Tab[2]) and np.array_equal(Tb[:2], Tab[:2])      # the record of stream 2 was consumed, and only that one
    # the records against numpy over the rows
    want_audit = et.audit_of_batch(r["tube_hist"], TOL)
    np.testing.assert_allclose(r["audit"], want_audit, rtol=0.0, atol=1e-11)
    want_track = bstream.track_of_rows(r["log_hist"], r["hist"])
    er.assert_track(r["track"], want_track, rtol=0.0, atol=1e-11)
    assert r["audit"][1, AUDIT["SAMPLES"]] == T and r["track"][0, TRACK["SAMPLES"]] == T


def test_sanitized_stand_alone_program():
    """the stand-alone program of the team rollout text under AddressSanitizer and UndefinedBehaviorSanitizer on the cases of emu_rollout.plain_cases,
    exact-size heap buffers: per case the plain and the fully-featured kernel under both wave orders, equal checksums"""
    out = er.run_sanitized(er.plain_cases(NW), NW)
    print("\n".join(out))
    assert len(out) == 5 and all(line.count("rc 0") == 4 and "DIFFERS" not in line for line in out)
    assert "ticks_run 6 of 6" in out[0] and "status 3" in out[1] and "ticks_run 4 of 4" in out[4]
