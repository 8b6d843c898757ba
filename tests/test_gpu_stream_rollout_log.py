"""GPU: the rollout with the log (bmpc_stream_rollout_log; StreamBatch.rollout(want_log=, log_stages=, track=)): the log rows of a rollout with a
disturbance and a spliced re-plan against the loop {one-wave fused tick, bmpc_stream_log, bmpc_stream_disturb, bmpc_stream_update(splice)} on a twin batch,
everything else against a rollout without the log, the tracking record against the numpy specification and against the g++ build of the same text, the
stopped streams, the argument errors.  (2, 2), B = 3 streams, T = 6, tick 0 solved out first unless said otherwise.
Bounds: the twin's rows come from the stand-alone log kernel, compiled in another unit than the rollout's log lines, so they are compared at
atol = rtol = 1e-11, the bound of tests/test_gpu_stream_log.py and tests/test_gpu_stream_tube.py for this text (device libm and contraction); the NaN
pattern and the trailer words exactly.  Measured on an MI355X the rows ARE the twin's, bit for bit (largest deviation 0 at both row lengths), and
that is asserted on top: the rollout's log lines and the stand-alone kernel compile to the same arithmetic at this shape.  The record's float slots against numpy on the GPU's own rows: rtol 1e-12 (tests/test_stream_rollout_log.py)."""
import numpy as np
import pytest

from tests.rollout_contract import assert_equal as _assert_equal, batch as _batch, close as _close, assert_track, contract_loop, cut, push, records as _records, small_streams as _small_streams, snapshot as _snapshot

pytestmark = pytest.mark.gpu
N, S, T = 2, 2, 6
ATOL = 1e-11
TOL = 1e-6
TICK_OF = np.array([-1, -1, 3])


def _assert_rows(got, want, what, exact=False):
    """log rows: the NaN pattern and the trailer words exact, the numbers to 1e-11 (exact: and bit for bit); returns the largest deviation"""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern"
    assert np.array_equal(got[..., -4:], want[..., -4:], equal_nan=True), f"{what}: trailer"
    dev = float(np.nanmax(np.abs(got - want))) if np.isfinite(got).any() else 0.0
    print(f"{what}: largest deviation {dev:.3e}, bit-equal {np.array_equal(got, want, equal_nan=True)}")
    np.testing.assert_allclose(got, want, rtol=ATOL, atol=ATOL, err_msg=what)
    assert not exact or np.array_equal(got, want, equal_nan=True), f"{what}: not bit for bit"
    return dev


def test_rollout_log_equals_the_tick_loop_and_changes_nothing_else():
    """the disturbance behind tick 2 of stream 1, a spliced re-plan behind tick 3 of stream 2: rollout(want_log, track) with rows of N stages and of one
    stage on two batches, the loop with log() on a one-wave twin, a fourth batch through rollout() without the log"""
    import torch
    from boundmpc_amd import stream as bstream
    TRACK = bstream.TRACK
    mpcs, recs = _small_streams(N, S)
    a, b, b1, c = (_batch(N, S, mpcs, recs, one_wave=True) for _ in range(4))
    for _, sb in (a, b, b1, c):
        sb.tick(max_iter=100, warm_dual=True)
    records, d = _records(mpcs, recs, a[1].entries), push(T, 3)
    kw = dict(max_iter=0, warm_dual=True)
    ev = dict(replan=records, replan_tick=TICK_OF, disturb=d)
    table0 = a[1].path.clone()
    rows = contract_loop(a[1], T, records, TICK_OF, d, want_log=True, **kw)["log_hist"]
    full = b[1].rollout(T, want_traj=True, audit=True, want_tube=True, audit_tol=TOL, want_log=True, log_stages=N, track=True, **ev, **kw)
    one = b1[1].rollout(T, want_traj=True, audit=True, want_tube=True, audit_tol=TOL, want_log=True, log_stages=1, track=True, **ev, **kw)
    plain = c[1].rollout(T, want_traj=True, audit=True, want_tube=True, audit_tol=TOL, **ev, **kw)
    torch.cuda.synchronize()
    lf, l1 = full["log_hist"].cpu().numpy(), one["log_hist"].cpu().numpy()
    assert lf.shape == (T, 3, 88 * N + 4) and l1.shape == (T, 3, 92) and full["ticks_run"].tolist() == [T] * 3 and full["replan_info"].tolist() == [-1, -1, 0]
    _assert_rows(lf, rows, "log_stages = N against the twin's log()", exact=True)
    _assert_rows(l1, cut(rows, N, 1), "log_stages = 1 against the twin's log()", exact=True)
    assert np.array_equal(l1, cut(lf, N, 1), equal_nan=True)         # the same lines of the same kernel: the prefix and the trailer, bit for bit
    assert (lf[:, [0, 2], -4] == N).all() and (lf[:4, 1, -4] == N).all() and not torch.equal(table0[2], b[1].path[2])
    # nothing else moves: the tick arrays, the tables, the record buffer, every returned tensor
    for got, sb in ((full, b[1]), (one, b1[1])):
        _assert_equal(_snapshot(sb), _snapshot(c[1]), "log on / off")
        _assert_equal(_snapshot(a[1]), _snapshot(sb), "tick loop / rollout with log")
        assert torch.equal(sb.path, c[1].path) and torch.equal(sb.replan, c[1].replan) and torch.equal(sb.path, a[1].path)
        for k in plain:
            assert np.array_equal(got[k].cpu().numpy(), plain[k].cpu().numpy(), equal_nan=True), k
    assert set(full) - set(plain) == {"log_hist", "track"}
    # the record: numpy on the GPU's own rows; it does not depend on the row length
    hist = full["hist"].cpu().numpy()
    trk = full["track"].cpu().numpy()
    assert_track(trk, bstream.track_of_rows(lf, hist))
    assert_track(one["track"].cpu().numpy(), bstream.track_of_rows(l1, hist))
    assert np.array_equal(trk, one["track"].cpu().numpy())
    print("stream 1:", bstream.unpack_track(trk[1]), "\nstream 0:", bstream.unpack_track(trk[0]))
    assert trk[0, TRACK["SAMPLES"]] == T and trk[1, TRACK["SAMPLES"]] == (lf[:, 1, -4] >= 1).sum() and trk[1, TRACK["TICK_EP_ORTH"]] >= 3
    # either array alone gives the same array; the record alone lives on a stage-0 row in LDS
    for kw2 in (dict(want_log=True, log_stages=1), dict(track=True)):
        e = _batch(N, S, mpcs, recs, one_wave=True)
        e[1].tick(max_iter=100, warm_dual=True)
        o2 = e[1].rollout(T, **kw2, **ev, **kw)
        torch.cuda.synchronize()
        _assert_equal(_snapshot(e[1]), _snapshot(c[1]), str(kw2))
        k = "track" if "track" in kw2 else "log_hist"
        assert ("track" in o2) == (k == "track") and ("log_hist" in o2) == (k == "log_hist") and "audit" not in o2
        assert np.array_equal(o2[k].cpu().numpy(), one[k].cpu().numpy(), equal_nan=True), k
        assert torch.equal(o2["hist"], plain["hist"])
        _close(e)
    _close(a, b, b1, c)


def test_rollout_log_on_the_gpu_equals_the_cpu_build_of_the_same_text():
    """From the cold start, converged with the dual state, the spliced re-plan behind tick 3 of stream 2 and pushes of every stream behind ticks 1 and 4
    (tests/emu/emu_rollout.py disturbances at a quarter of their scale: with this re-plan schedule the full ones leave stream 0 unconverged at
    the last tick): rows and record against tests/emu's g++ build of the kernel text, 1e-11.
    Why not the 0.01 rad push of the test above: across two BUILDS only converged solves are comparable.  Behind that push stream 1 is outside its tube
    and its solves end unconverged (status 2, KKT 1e-3 .. 0.2); the two builds then stop at iterates 1.9e-6 apart in the robot record of `hist` itself,
    and the rows inherit 1.6e-8 (measured on an MI355X; every converged tick of the same run agrees to 1.1e-15).  That is the solver's spread, not the
    log's; the log of those ticks is checked against the twin above, which runs the same solver build.  So every tick here must converge, and that is
    asserted."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu, emu_rollout as ee
    mpcs, recs = _small_streams(N, S)
    g = _batch(N, S, mpcs, recs)
    records, d = _records(mpcs, recs, g[1].entries), ee.disturbances(T, 3, on=(1, 4), scale=(5e-4, 1.25e-3, 2.5e-3))
    out = g[1].rollout(T, warm_dual=True, replan=records, replan_tick=TICK_OF, disturb=d, want_log=True, log_stages=N, track=True)
    torch.cuda.synchronize()
    _, A, Tab, R = ee.small_batch(N, S)
    assert np.array_equal(R, records)
    r = ee.rollout(N, S, 0.1, Tab, A, T, entry=3, replan=R, replan_tick=TICK_OF, disturb=d, opts=emu.opts_for(N, start_rollout=0), log_stages=N)
    assert out["ticks_run"].tolist() == r["ticks_run"].tolist() == [T] * 3 and out["replan_info"].tolist() == r["replan_info"].tolist() == [-1, -1, 0]
    assert (out["hist"].cpu().numpy()[:, :, bstream.ROLL["STATUS"]] == 0).all() and (r["hist"][:, :, bstream.ROLL["STATUS"]] == 0).all()
    log = out["log_hist"].cpu().numpy()
    _assert_rows(log, r["log_hist"], "GPU against the g++ build")
    # the record: against the g++ build's, and against the specification on the g++ build's rows
    trk = out["track"].cpu().numpy()
    assert_track(trk, r["track"], rtol=ATOL, atol=ATOL)
    assert_track(trk, bstream.track_of_rows(cut(r["log_hist"], N, 1), r["hist"]), rtol=ATOL, atol=ATOL)
    assert_track(trk, bstream.track_of_rows(log, out["hist"].cpu().numpy()))
    _close(g)


def test_stopped_streams_in_the_log():
    """a stream lost on entry and a stream that stops at its goal inside the launch (the tolerance from the batch's own phi trace); then plants pushed
    16 cm off their paths at one iteration a tick (the forced failures of tests/test_stream_rollout_events.py): a tick that ran and exhausted the plan"""
    import torch
    from boundmpc_amd import stream as bstream
    ROLL, SS, TRACK = bstream.ROLL, bstream.SS, bstream.TRACK
    mpcs, recs = _small_streams(N, S)
    a, b = _batch(N, S, mpcs, recs), _batch(N, S, mpcs, recs)
    for _, sb in (a, b):
        sb.state[2, SS["ERRCNT"]] = float(N)
    trace = a[1].rollout(T, warm_dual=True)
    torch.cuda.synchronize()
    gap = a[1].state[:, SS["PHIMAX"]].cpu().numpy()[None] - trace["hist"].cpu().numpy()[:, :, ROLL["PHI"]]
    goal = float(gap[1, 0])                                        # stream 0 stops behind tick 1
    want = [int(np.argmax(gap[:, i] <= goal)) + 1 if (gap[:, i] <= goal).any() else T for i in range(2)] + [0]
    out = b[1].rollout(T, warm_dual=True, goal_tol=goal, want_log=True, log_stages=N, track=True)
    torch.cuda.synchronize()
    log, trk, run = out["log_hist"].cpu().numpy(), out["track"].cpu().numpy(), out["ticks_run"].tolist()
    assert run == want and run[0] == 2 and run[2] == 0
    for i in range(3):
        assert np.isfinite(log[:run[i], i]).all() and np.isnan(log[run[i]:, i]).all() and trk[i, TRACK["SAMPLES"]] == run[i]
    assert (trk[2, [1, 4, 7]] == -np.inf).all() and (trk[2, [2, 5, 8]] == -1).all() and (trk[2, [0, 3, 6, 9, 10, 11]] == 0).all()
    assert_track(trk, bstream.track_of_rows(log, out["hist"].cpu().numpy()))
    _close(a, b)
    # exhausted mid-run
    c = _batch(N, S, mpcs, recs, one_wave=True)
    c[1].tick(max_iter=100, warm_dual=True)
    push = np.zeros((3, 21)); push[:, :4] = [0.1, -0.1, 0.1, 0.1]
    c[1].disturb(push)
    out = c[1].rollout(T, max_iter=1, warm_dual=True, want_log=True, log_stages=N, track=True)
    torch.cuda.synchronize()
    log, trk, run, hist = out["log_hist"].cpu().numpy(), out["track"].cpu().numpy(), out["ticks_run"].tolist(), out["hist"].cpu().numpy()
    assert run == [2, 2, 2] and (hist[1, :, ROLL["ERRCNT"]] == N).all() and (hist[0, :, ROLL["ERRCNT"]] == 1).all()
    assert (log[1, :, -4] == 0).all() and (log[1, :, -3] == N).all() and (log[1, :, -2:] == 0).all() and np.isnan(log[1, :, :-4]).all()      # ran, and no sample
    assert (log[0, :, -4] == 1).all() and np.isfinite(log[0, :, :88]).all() and np.isnan(log[0, :, 88:-4]).all() and np.isnan(log[2:]).all()
    assert (trk[:, TRACK["SAMPLES"]] == 1).all() and (trk[:, [2, 5, 8]] == 0).all()
    assert_track(trk, bstream.track_of_rows(log, hist))
    assert bstream.unpack_log(log[1, 0], N, stages=N) == (None, None) and bstream.unpack_log(log[3, 0], N, stages=N) == (None, None)
    _close(c)


def test_argument_errors_and_lengths():
    import torch
    from boundmpc_amd import stream as bstream
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    mpcs, recs = _small_streams(N, S)
    solver, sb = _batch(N, S, mpcs, recs)
    L = solver._lib
    assert L.bmpc_stream_track_len() == bstream.track_len() == 12
    assert [L.bmpc_stream_rollout_log_len(solver._h, k) for k in (1, N)] == [92, 88 * N + 4] == [bstream.rollout_log_len(1), bstream.rollout_log_len(N)]
    assert all(L.bmpc_stream_rollout_log_len(solver._h, k) <= 0 for k in (0, N + 1, -1)) and L.bmpc_stream_rollout_log_len(None, 1) <= 0
    dev = sb.path.device
    torch.cuda.synchronize()
    before = _snapshot(sb)
    t = {k: getattr(sb, k) for k in before}
    log, track = torch.full((2, 3, 88 * N + 4), 7.0, dtype=torch.float64, device=dev), torch.full((3, 12), 7.0, dtype=torch.float64, device=dev)

    def raw(ticks=2, flags=1, goal=0.0, uflags=3, tol=1e-6, lg=log, stages=1, tr=track, replan=None):
        return L.bmpc_stream_rollout_log(solver._h, 3, ticks, _ptr(sb.path), sb.entries, _ptr(t["state"]), _ptr(t["robot"]), _ptr(t["p"]), _ptr(t["x0"]), _ptr(t["dual"]),
                                         0, _ptr(t["x"]), _ptr(t["g"]), _ptr(t["iters"]), _ptr(t["status"]), _ptr(t["kkt"]), _ptr(t["traj"]), flags, goal, None, None,
                                         None, _ptr(replan), None, None, uflags, None, None, None, tol, _ptr(lg), stages, _ptr(tr), None)
    for stages in (0, N + 1, -1):
        for kw in (dict(), dict(lg=None), dict(tr=None)):
            assert raw(stages=stages, **kw) == 1, (stages, kw)
    for kw in (dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=-1.0, lg=None, tr=None), dict(ticks=0), dict(flags=0), dict(goal=-1.0), dict(uflags=8), dict(replan=track)):
        assert raw(**kw) == 1, kw
    with pytest.raises(ValueError):
        sb.rollout(2, warm_dual=True, want_log=True, log_stages=N + 1)
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(2, warm_dual=True, track=True, log_stages=0)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert (log == 7.0).all() and (track == 7.0).all()
    _close((solver, sb))
