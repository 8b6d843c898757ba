"""CPU: the rollout with the log (csrc/bmpc_rollout_kernel.inl with LG, bmpc_stream_rollout_log) as a g++ build of its own text (tests/emu): the log rows
of an emulated rollout with a disturbance and a spliced re-plan against the per-tick loop {tick text, log text cut to the stages, disturb text, update
text}, bit for bit (the same text under the same compiler); everything else against the rollout without the log; the tracking record against the numpy
specification boundmpc_amd.stream.track_of_rows.
Tolerance of the record's float slots: rtol 1e-12, derived, not measured -- a sum of squares is at most T additions of terms that may each carry one
contraction, well under T 2^-52 relative for T = 6; the integer slots (samples, ticks, replayed) are compared exactly."""
import functools

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_stream_log as el, emu_stream_update as eup

ROLL, SS, TRACK, LS = bstream.ROLL, bstream.SS, bstream.TRACK, bstream.LOG_STAGE
N, S, T, H = 2, 2, 6, 0.1
TOL = 1e-6
REPLAN_TICK = np.array([-1, -1, 3])
OUTPUTS = ("hist", "traj_hist", "ticks_run", "replan_info", "tube_hist", "audit")


_copy = er.copy_arrays


def _run(entry=3, A0=None, disturb=True, replan=True, **kw):
    """one emulated rollout of T ticks on copies of the start -> (result, tick arrays, tables, records)"""
    A0_, Tab, recs = er.start(N, S)
    A, Tb, R = _copy(A0_ if A0 is None else A0), Tab.copy(), recs.copy()
    ev = dict(replan=R, replan_tick=REPLAN_TICK, update_flags=3) if replan else {}
    r = er.rollout(N, S, H, Tb, A, T, entry=entry, disturb=er.push(T, 3) if disturb else None, opts=er.opts(N), audit_tol=TOL, **ev, **kw)
    return r, A, Tb, R


@functools.lru_cache(maxsize=None)
def _rollouts():
    """the disturbance behind tick 2 of stream 1, a spliced re-plan behind tick 3 of stream 2: the rollout with rows of N stages, with rows of one stage,
    the rollout with the audit alone, and per stream the per-tick loop for both row lengths -- computed once"""
    full, one, off = _run(log_stages=N), _run(log_stages=1), _run(2)
    A0, Tab, recs = er.start(N, S)
    d = er.push(T, 3)
    loops = {}
    for stages in (1, N):
        per = [er.contract_loop(N, S, H, Tab[b].copy(), er.unstack(A0, b), T, stages, replan=recs[b].copy(), replan_tick=int(REPLAN_TICK[b]), update_flags=3,
                                disturb=d[:, b], opts=er.opts(N)) for b in range(3)]
        loops[stages] = (np.stack([p["log_hist"] for p in per], axis=1), np.stack([p["hist"] for p in per], axis=1))
    return full, one, off, loops


def test_slot_maps_and_lengths():
    assert bstream.track_len() == TRACK["LEN"] == 12 and sorted(v for k, v in TRACK.items() if k != "LEN") == list(range(11))
    assert [er.rollout_log_len(N, k) for k in (1, N)] == [bstream.rollout_log_len(1), bstream.rollout_log_len(N)] == [92, 88 * N + 4] and bstream.rollout_log_len(N) == bstream.log_len(N)
    row = np.zeros(12); row[[0, 1, 2, 3, 5, 8, 10]] = [4.0, 0.5, 2.0, 1.0, -1.0, -1.0, 3.0]
    u = bstream.unpack_track(row)
    assert u["samples"] == 4 and u["max_e_p_orth"] == 0.5 and u["tick_e_p_orth"] == 2 and u["rms_e_p_orth"] == 0.5 and u["tick_e_p_par"] is None and u["tick_e_r"] is None and u["replayed"] == 3
    assert np.isnan(bstream.unpack_track(np.zeros(12))["rms_e_r"])


def test_log_rows_equal_the_per_tick_loop():
    (full, _, Tb, R), (one, _, _, _), _, loops = _rollouts()
    assert full["ran"] == one["ran"] == 3 and full["ticks_run"].tolist() == [T] * 3 and full["replan_info"].tolist() == [-1, -1, 0]
    assert np.array_equal(full["hist"], loops[N][1], equal_nan=True)
    assert full["log_hist"].shape == (T, 3, 88 * N + 4) and one["log_hist"].shape == (T, 3, 92)
    assert np.array_equal(full["log_hist"], loops[N][0], equal_nan=True) and np.array_equal(one["log_hist"], loops[1][0], equal_nan=True)      # bit for bit
    # the short rows are the prefix and the trailer of the long ones; n_valid is the whole plan's
    assert np.array_equal(one["log_hist"][..., :LS], full["log_hist"][..., :LS], equal_nan=True) and np.array_equal(one["log_hist"][..., -4:], full["log_hist"][..., -4:])
    calm = [0, 2]                                                   # (the pushed stream fails ticks behind the push: shorter plans, see below)
    assert (one["log_hist"][:, calm, -4] == N).all() and (one["log_hist"][:, calm, -3] == 0).all() and np.isfinite(full["log_hist"][:, calm]).all()
    assert (full["log_hist"][:4, 1, -4] == N).all() and np.array_equal(full["log_hist"][:, 1, -4] + full["log_hist"][:, 1, -3], np.full(T, float(N)))
    ref, err = bstream.unpack_log(one["log_hist"][4, 0], N, stages=1)
    assert len(err["e_p_orth"]) == 1 and np.array_equal(err["e_p_orth"][0], full["log_hist"][4, 0, 55 + 9:55 + 12]) and len(bstream.unpack_log(full["log_hist"][4, 0], N)[0]["p"]) == N
    # the row of the re-plan tick is the one taken BEFORE the table was rewritten: the loop stopped behind that tick holds the rewritten table, and the log
    # text on it gives another row
    A0, Tab, recs = er.start(N, S)
    A2, T2 = er.unstack(A0, 2), Tab[2].copy()
    rows = er.contract_loop(N, S, H, T2, A2, 4, N, replan=recs[2].copy(), replan_tick=3, update_flags=3, opts=er.opts(N))["log_hist"]
    assert np.array_equal(T2, Tb[2]) and not np.array_equal(T2, Tab[2])
    behind = er.cut(el.stream_log(N, S, H, T2, A2["ss"], A2["p"], A2["traj"]), N, N)
    assert np.array_equal(rows[3], full["log_hist"][3, 2]) and not np.array_equal(behind, full["log_hist"][3, 2], equal_nan=True)


def test_the_log_changes_nothing_else():
    (full, A, Tb, R), (one, A1, Tb1, R1), (off, A_off, Tb_off, R_off), _ = _rollouts()
    for got_r, got_A, got_T, got_R in ((full, A, Tb, R), (one, A1, Tb1, R1)):
        for k in got_A:
            assert np.array_equal(got_A[k], A_off[k], equal_nan=True), k
        assert np.array_equal(got_T, Tb_off) and np.array_equal(got_R, R_off)
        for k in OUTPUTS:
            assert np.array_equal(got_r[k], off[k], equal_nan=True), k


def test_either_array_alone_and_neither():
    (full, _, _, _), (one, _, _, _), (off, A_off, Tb_off, R_off), _ = _rollouts()
    for kw, ran in ((dict(want_log=False), 3), (dict(track=False), 3), (dict(want_log=False, track=False), 2), (dict(want_log=False, track=False, audit=False, want_tube=False), 1)):
        r, A, Tb, R = _run(log_stages=1, **kw)
        assert r["ran"] == ran, kw
        for k in A:
            assert np.array_equal(A[k], A_off[k], equal_nan=True), (kw, k)
        assert np.array_equal(Tb, Tb_off) and np.array_equal(R, R_off)
        for k in OUTPUTS:
            if r[k] is not None:
                assert np.array_equal(r[k], off[k], equal_nan=True), (kw, k)
        for k in ("log_hist", "track"):
            if r[k] is not None:
                assert np.array_equal(r[k], one[k], equal_nan=True), (kw, k)
    assert np.array_equal(one["track"], full["track"])      # the record does not depend on the row length, nor on where the row lives


def test_track_equals_the_numpy_specification():
    (full, _, _, _), (one, _, _, _), _, _ = _rollouts()
    for r in (full, one):
        er.assert_track(r["track"], bstream.track_of_rows(r["log_hist"], r["hist"]))
    trk = full["track"]
    assert (trk[[0, 2], TRACK["SAMPLES"]] == T).all() and (trk[:, 11] == 0).all() and (trk[[0, 2], TRACK["REPLAYED"]] == 0).all()
    sample = full["log_hist"][:, 1, -4] >= 1                       # (the last tick of the pushed stream exhausts its plan: a replay that is no sample)
    assert trk[1, TRACK["SAMPLES"]] == sample.sum() == T - 1 and trk[1, TRACK["REPLAYED"]] == (full["hist"][sample, 1, ROLL["USINGPREV"]] > 0).sum() == 1
    calm, _, _, _ = _run(disturb=False, want_log=False, log_stages=1)
    u, c = bstream.unpack_track(trk[1]), bstream.unpack_track(calm["track"][1])
    print("stream 1, disturbed:", u, "\nstream 1, undisturbed:", c)
    assert u["max_e_p_orth"] > c["max_e_p_orth"] and u["tick_e_p_orth"] >= 3 and u["rms_e_p_orth"] > c["rms_e_p_orth"]
    assert np.array_equal(trk[0], calm["track"][0])      # the streams are independent
    # every rule of the specification on made-up rows: the first of equal maxima, a non-finite norm, rows without a sample, replays
    rows, hist = np.full((5, 1, 92), np.nan), np.zeros((5, 1, ROLL["LEN"]))
    for t, (eo, nv, up) in enumerate([(3.0, 2, 0), (4.0, 1, 1), (4.0, 2, 1), (np.inf, 0, 1), (np.nan, 2, 0)]):
        rows[t, 0, :88], rows[t, 0, 88:] = 0.0, (nv, 0, 0, 0)
        rows[t, 0, 55 + 9], rows[t, 0, 55 + 19], hist[t, 0, ROLL["USINGPREV"]] = eo, 0.5 * t, up
    w = bstream.track_of_rows(rows[:4], hist[:4])[0]
    assert w[:4].tolist() == [3.0, 4.0, 1.0, 41.0] and w[4:7].tolist() == [0.0, 0.0, 0.0] and w[7:].tolist() == [1.0, 2.0, 1.25, 2.0, 0.0]
    w = bstream.track_of_rows(rows, hist)[0]
    assert w[0] == 4 and np.isnan(w[1]) and w[2] == 4 and np.isnan(w[3]) and w[7:10].tolist() == [2.0, 4.0, 5.25]


def test_stopped_streams():
    """a stream lost on entry, a stream that stops at its goal inside the launch (the cold start and the tolerance of tests/test_stream_tube.py), and a
    stream whose plan a post exhausts mid-run (the forced failures of tests/test_stream_rollout_events.py: plants pushed 16 cm off their paths, one
    iteration a tick)"""
    _, A0, Tab, _ = er.small_batch(N, S)
    A = _copy(A0)
    A["ss"][2, SS["ERRCNT"]] = float(N)
    r = er.rollout(N, S, H, Tab.copy(), A, T, entry=3, opts=er.opts(N), goal_tol=6.9242, log_stages=N)
    run = r["ticks_run"].tolist()
    assert 0 < run[0] < T and run[2] == 0
    for b in range(3):
        assert np.isfinite(r["log_hist"][:run[b], b]).all() and np.isnan(r["log_hist"][run[b]:, b]).all()      # (the trailer included)
        assert r["track"][b, TRACK["SAMPLES"]] == run[b]
    lost = r["track"][2]
    assert lost[TRACK["SAMPLES"]] == 0 and (lost[[1, 4, 7]] == -np.inf).all() and (lost[[2, 5, 8]] == -1).all() and (lost[[3, 6, 9, 10, 11]] == 0).all()
    er.assert_track(r["track"], bstream.track_of_rows(r["log_hist"], r["hist"]))
    # exhausted mid-run
    A0, Tab, _ = er.start(N, S)
    A = _copy(A0)
    push = np.zeros(21); push[:4] = [0.1, -0.1, 0.1, 0.1]
    for b in range(3):
        A["rb"][b] = eup.stream_disturb(A["rb"][b], push)
    loop = er.contract_loop(N, S, H, Tab[0].copy(), er.unstack(A, 0), T, N, max_iter=1, opts=er.opts(N))["log_hist"]
    r = er.rollout(N, S, H, Tab.copy(), A, T, entry=3, opts=er.opts(N), max_iter=1, log_stages=N)
    assert r["ticks_run"].tolist() == [2, 2, 2] and r["hist"][:2, 0, ROLL["ERRCNT"]].tolist() == [1, 2]
    assert np.array_equal(r["log_hist"][:, 0], loop, equal_nan=True)
    row = r["log_hist"][1, 0]                                      # a tick that RAN, and whose post exhausted the plan
    assert row[-4:].tolist() == [0.0, float(N), 0.0, 0.0] and np.isnan(row[:-4]).all() and bstream.unpack_log(row, N, stages=N) == (None, None)
    assert r["log_hist"][0, 0, -4] == 1 and np.isfinite(r["log_hist"][0, 0, :LS]).all() and np.isnan(r["log_hist"][0, 0, LS:-4]).all()
    assert (r["track"][:, TRACK["SAMPLES"]] == 1).all() and (r["track"][:, [2, 5, 8]] == 0).all() and np.isnan(r["log_hist"][2:]).all()
    er.assert_track(r["track"], bstream.track_of_rows(r["log_hist"], r["hist"]))
    assert bstream.unpack_log(r["log_hist"][3, 0], N, stages=N) == (None, None)      # a tick the stream did not run


def test_argument_refusals_mirror_the_entry():
    A0, Tab, _ = er.start(N, S)
    A = _copy(A0)
    call = lambda **kw: er.rollout(N, S, H, Tab.copy(), A, kw.pop("ticks", T), entry=3, opts=er.opts(N), want_rc=True, **kw)
    for stages in (0, N + 1, -1):
        for kw in (dict(), dict(want_log=False), dict(track=False)):
            assert call(log_stages=stages, **kw) == 1, (stages, kw)
    for kw in (dict(audit_tol=-1.0), dict(ticks=0), dict(simulate=False), dict(goal_tol=-1.0), dict(update_flags=8), dict(replan=np.zeros((3, bstream.replan_len(S, Tab.shape[1])))),
               dict(audit_tol=-1.0, want_log=False, track=False)):
        assert call(**kw) == 1, kw
    for k in A:
        assert np.array_equal(A[k], A0[k], equal_nan=True), k      # nothing ran
    assert [er.rollout_log_len(N, k) for k in (0, N + 1, -3)] == [-1, -1, -1]
    with pytest.raises(AssertionError):
        bstream.unpack_log(np.zeros(92), N)                       # the default keeps the whole-row assertion
    with pytest.raises(AssertionError):
        bstream.unpack_log(np.zeros(92), N, stages=N)


def test_sanitized_stand_alone_program():
    """the stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer on the four cases of the rollout with the audit, exact-size buffers"""
    out = er.run_sanitized(er.plain_cases(1, only=(3,)), 1)      # (the one program of the one-wave texts: its cases with the log, at that level)
    print("\n".join(out))
    assert len(out) == 4 and all("rc 0 ran 3" in line and "| rc 0 ran 3" in line for line in out)


def test_the_reference_shape_equals_the_per_tick_loop():
    """(10, 4): three ticks of one recorded-experiment stream with rows of all ten stages, the instantiation with the iterate in LDS -- the log's LDS words
    at the product's shape"""
    Nn, Sn, ticks = 10, 4, 3
    _, rec, Tab, ss = er.small_stream(Nn, Sn)
    A0 = er.fresh_arrays(Nn, Sn, ss, rec)
    opts = emu.opts_for(Nn, start_rollout=0)
    A = er.stack([A0])
    r = er.rollout(Nn, Sn, H, np.ascontiguousarray(Tab[None]), A, ticks, entry=3, opts=opts, log_stages=Nn)
    loop = er.contract_loop(Nn, Sn, H, Tab.copy(), er.copy_arrays(A0), ticks, Nn, opts=opts)
    rows, hist = loop["log_hist"], loop["hist"]
    assert r["ticks_run"].tolist() == [ticks] and np.array_equal(r["hist"][:, 0], hist, equal_nan=True)
    assert np.array_equal(r["log_hist"][:, 0], rows, equal_nan=True) and np.isfinite(rows).all() and (rows[:, -4] == Nn).all()
    er.assert_track(r["track"], bstream.track_of_rows(r["log_hist"], r["hist"]))
