"""GPU: the tube measurement on the device (bmpc_stream_tube; StreamBatch.tube) and the rollout with the audit (bmpc_stream_rollout_audit;
StreamBatch.rollout(audit=, want_tube=)): the service launch against the g++ build of the same text, the audit of a disturbed rollout against the loop
{one-wave fused tick, tube launch, bmpc_stream_disturb} on a twin and against a rollout without audit, the tube launch captured behind a tick, the
argument errors.  (2, 2), B = 3 streams; the rows of the recorded experiments need a (10, 4) handle."""
import numpy as np
import pytest

from tests.rollout_contract import assert_equal as _assert_equal, batch as _batch, close as _close, push, small_streams as _small_streams, snapshot as _snapshot

pytestmark = pytest.mark.gpu
N, S = 2, 2
ATOL = 1e-11                     # the bound of the log, update and rollout GPU tests: device libm and contraction against the host's
TOL = 1e-6


def _raw_tube(solver, B, p, state, out):
    from boundmpc_amd.solver import _ptr
    return solver._lib.bmpc_stream_tube(solver._h, B, _ptr(p), _ptr(state), _ptr(out), None)


def test_service_launch_equals_the_cpu_build():
    """the hand-made rows and every p of the recorded experiments, uploaded: 1e-11 against the g++ build, the segment exact; state rows without a plan"""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    from tests.emu import emu_stream_tube as et
    TUBE = bstream.TUBE
    p = np.concatenate([np.stack(list(et.hand_made().values())), et.g7_p(), et.g14_p()])
    want = et.stream_tube(10, 4, p)
    solver = BatchedOCPSolver(10, 4, 0.1)
    assert solver._lib.bmpc_stream_tube_len() == bstream.tube_len() == 16
    dev = torch.device("cuda")
    pd, out = torch.as_tensor(p, device=dev), torch.full((len(p), 16), 7.0, dtype=torch.float64, device=dev)
    assert _raw_tube(solver, len(p), pd, None, out) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    dev_ = et.deviations(got, want)      # (asserts the NaN slots and the segments equal)
    print("largest deviation GPU - CPU build per slot group:", "  ".join(f"{k} {v:.3e}" for k, v in dev_.items()))
    assert max(dev_.values()) <= ATOL
    assert (got[:, TUBE["EX_ROT"]] > 1e-3).any() and np.isnan(got[4, TUBE["EX_POS"]]) and 0.03 < got[1, TUBE["EX_POS"]] < 0.05
    # state rows: error counts N, N - 1, NaN
    ss = np.zeros((3, bstream.ss_len(10))); ss[:, bstream.SS["ERRCNT"]] = [10.0, 9.0, np.nan]
    out3 = torch.full((3, 16), 7.0, dtype=torch.float64, device=dev)
    assert _raw_tube(solver, 3, pd[[0, 0, 0]].contiguous(), torch.as_tensor(ss, device=dev), out3) == 0
    torch.cuda.synchronize()
    o = out3.cpu().numpy()
    assert np.isnan(o[0]).all() and np.isnan(o[2]).all() and np.array_equal(o[1], got[0])
    solver.close()


def test_rollout_audit_equals_the_tick_loop_and_changes_nothing_else():
    """Tick 0 solved out, then T = 6 with the disturbance behind tick 2 of stream 1: rollout(audit, want_tube) on one batch; on a one-wave twin T
    launches of tick(), the tube launch behind each (row t: the p tick t packed) and disturb(); a third batch through rollout() without audit."""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_stream_tube as et
    TUBE, AUDIT, SS, T = bstream.TUBE, bstream.AUDIT, bstream.SS, 6
    mpcs, recs = _small_streams(N, S)
    a, b, c = (_batch(N, S, mpcs, recs, one_wave=True) for _ in range(3))
    for _, sb in (a, b, c):
        sb.tick(max_iter=100, warm_dual=True)
    d = push(T, 3)
    kw = dict(max_iter=0, warm_dual=True)
    # the loop on the twin
    sb = a[1]
    rows = np.full((T, 3, 16), np.nan)
    raw = torch.empty((3, 16), dtype=torch.float64, device=sb.path.device)
    for t in range(T):
        lost = sb.state[:, SS["ERRCNT"]].cpu().numpy() >= N
        sb.tick(simulate=True, **kw)
        by_method = sb.tube().clone()                              # (NaN for a stream whose plan THIS tick's post exhausted: its state row says so)
        assert _raw_tube(a[0], 3, sb.p, None, raw) == 0
        torch.cuda.synchronize()
        row = raw.cpu().numpy().copy()
        plan = sb.has_plan().cpu().numpy()
        assert np.array_equal(by_method.cpu().numpy()[plan], row[plan]) and np.isnan(by_method.cpu().numpy()[~plan]).all()
        row[lost] = np.nan
        rows[t] = row
        dt = d[t].copy(); dt[lost] = 0.0
        sb.disturb(dt)
    torch.cuda.synchronize()
    out = b[1].rollout(T, disturb=d, audit=True, want_tube=True, audit_tol=TOL, **kw)
    plain = c[1].rollout(T, disturb=d, **kw)
    torch.cuda.synchronize()
    tube, audit = out["tube_hist"].cpu().numpy(), out["audit"].cpu().numpy()
    assert np.array_equal(tube, rows, equal_nan=True)                                       # bit for bit
    assert np.array_equal(audit, et.audit_of_batch(tube, TOL), equal_nan=True)
    _assert_equal(_snapshot(b[1]), _snapshot(c[1]), "audit on / off")
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "tick loop / rollout with audit")
    assert np.array_equal(out["hist"].cpu().numpy(), plain["hist"].cpu().numpy(), equal_nan=True)
    assert out["ticks_run"].tolist() == plain["ticks_run"].tolist()
    ex = tube[:, :, TUBE["EX_POS"]]
    print("position excess of stream 1 per tick:", ex[:, 1], " audit:", bstream.unpack_audit(audit[1]))
    assert ex[3, 1] > 1e-3 > TOL and (ex[:3] < 0).all()
    a1 = bstream.unpack_audit(audit[1])
    assert a1["first_out"] == 3 and a1["tick_pos"] == 3 and a1["max_pos"] == ex[3, 1] and a1["samples"] == int(out["ticks_run"][1])
    assert bstream.unpack_audit(audit[0])["first_out"] is None and audit[0, AUDIT["SAMPLES"]] == int(out["ticks_run"][0])
    # either array alone gives the same array
    for kw2 in (dict(audit=True), dict(want_tube=True)):
        e = _batch(N, S, mpcs, recs, one_wave=True)
        e[1].tick(max_iter=100, warm_dual=True)
        o2 = e[1].rollout(T, disturb=d, audit_tol=TOL, **kw2, **kw)
        torch.cuda.synchronize()
        _assert_equal(_snapshot(e[1]), _snapshot(c[1]), str(kw2))
        k = "audit" if "audit" in kw2 else "tube_hist"
        assert ("audit" in o2) == (k == "audit") and ("tube_hist" in o2) == (k == "tube_hist")
        assert np.array_equal(o2[k].cpu().numpy(), out[k].cpu().numpy(), equal_nan=True), k
        _close(e)
    _close(a, b, c)


def test_stopped_streams_in_the_audit():
    """a stream lost on entry: NaN rows, SAMPLES 0, maxima -inf, FIRST_OUT -1; the others audited on every tick they ran"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_stream_tube as et
    AUDIT, T = bstream.AUDIT, 3
    mpcs, recs = _small_streams(N, S)
    g = _batch(N, S, mpcs, recs)
    g[1].state[2, bstream.SS["ERRCNT"]] = float(N)
    out = g[1].rollout(T, warm_dual=True, audit=True, want_tube=True)
    torch.cuda.synchronize()
    tube, audit, run = out["tube_hist"].cpu().numpy(), out["audit"].cpu().numpy(), out["ticks_run"].tolist()
    assert run == [T, T, 0] and np.isnan(tube[:, 2]).all() and not np.isnan(tube[:, :2]).any()
    assert audit[2, AUDIT["SAMPLES"]] == 0 and audit[2, AUDIT["FIRST_OUT"]] == -1 and (audit[2, [1, 3, 5, 6]] == -np.inf).all()
    assert np.array_equal(audit, et.audit_of_batch(tube, 1e-6), equal_nan=True)
    _close(g)


def test_tube_launch_captured_behind_a_tick():
    """{tick, tube} captured on the caller's stream and replayed once, against the direct calls on a twin"""
    import torch
    mpcs, recs = _small_streams(N, S)
    a, b = _batch(N, S, mpcs, recs, one_wave=True), _batch(N, S, mpcs, recs, one_wave=True)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _, sb in (a, b):
            sb.tick(max_iter=100, warm_dual=True)
            sb.tube()                                              # (allocates the buffer ahead of the capture)
        side.synchronize()
        a[1].tick(simulate=True, warm_dual=True); want = a[1].tube()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            b[1].tick(simulate=True, warm_dual=True); got = b[1].tube()
        graph.replay()
        side.synchronize()
    assert torch.equal(want, got) and not torch.isnan(got).any()
    _assert_equal(_snapshot(a[1]), _snapshot(b[1]), "direct / replayed")
    del graph
    torch.cuda.synchronize()
    _close(a, b)


def test_argument_errors_of_both_entries():
    import torch
    from boundmpc_amd._lib import BoundMPCHipError
    from boundmpc_amd.solver import _ptr
    mpcs, recs = _small_streams(N, S)
    solver, sb = _batch(N, S, mpcs, recs)
    dev = sb.path.device
    out = torch.full((3, 16), 7.0, dtype=torch.float64, device=dev)
    assert _raw_tube(solver, 0, sb.p, sb.state, out) == 1 and _raw_tube(solver, -1, sb.p, sb.state, out) == 1
    assert _raw_tube(solver, 3, None, sb.state, out) == 1 and _raw_tube(solver, 3, sb.p, sb.state, None) == 1
    assert solver._lib.bmpc_stream_tube(None, 3, _ptr(sb.p), None, _ptr(out), None) == 1
    torch.cuda.synchronize()
    before = _snapshot(sb)
    t = {k: getattr(sb, k) for k in before}
    tube, audit = torch.full((2, 3, 16), 7.0, dtype=torch.float64, device=dev), torch.full((3, 12), 7.0, dtype=torch.float64, device=dev)

    def raw(ticks=2, flags=1, goal=0.0, uflags=3, tol=1e-6, th=tube, au=audit, replan=None):
        return solver._lib.bmpc_stream_rollout_audit(solver._h, 3, ticks, _ptr(sb.path), sb.entries, _ptr(t["state"]), _ptr(t["robot"]), _ptr(t["p"]), _ptr(t["x0"]), _ptr(t["dual"]),
                                                     0, _ptr(t["x"]), _ptr(t["g"]), _ptr(t["iters"]), _ptr(t["status"]), _ptr(t["kkt"]), _ptr(t["traj"]), flags, goal, None, None,
                                                     None, _ptr(replan), None, None, uflags, None, _ptr(th), _ptr(au), tol, None)
    for kw in (dict(tol=-1e-9), dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=-1.0, th=None, au=None), dict(ticks=0), dict(flags=0), dict(goal=-1.0), dict(uflags=8),
               dict(replan=out)):
        assert raw(**kw) == 1, kw
    with pytest.raises(BoundMPCHipError, match="invalid argument"):
        sb.rollout(2, warm_dual=True, audit=True, audit_tol=-1.0)
    torch.cuda.synchronize()
    _assert_equal(before, _snapshot(sb), "nothing was launched")
    assert (tube == 7.0).all() and (audit == 7.0).all() and (out == 7.0).all()
    _close((solver, sb))
