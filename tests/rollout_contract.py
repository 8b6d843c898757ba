"""What the GPU tests of the rollouts (tests/test_gpu_stream_*rollout*.py, tests/test_gpu_stream_tube.py) and their diagnostic scripts share: small
batches with a twin, snapshots of the tick arrays, and the contract's loop on a batch -- per tick {fused tick, [tube], [log], disturb, update of the
records due} with the rollout's stop rules -- that is the exact checker of every rollout variant (on one wave per stream or, with set_team_waves(4), on
teams).  The CPU twin of the loop, on the g++ build of the same kernel text: tests/emu/emu_rollout.py contract_loop.  No test in here."""
import numpy as np

from tests.emu.emu_rollout import assert_track, cut, push      # noqa: F401  (pure numpy: the GPU tests take them from here)

ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")
HELD = dict(tol=1e-3, max_iter=30, fixed_barrier="auto", bound_margin=2e-3)      # the held-barrier real-time mode bench.py reports for configs[4]


def small_streams(N, S, n=3):
    from tests.emu import emu_rollout as er
    made = [er.small_stream(N, S, which=i) for i in range(n)]
    return [m[0] for m in made], np.stack([m[1] for m in made])


def batch(N, S, mpcs, recs, one_wave=False, held=False, **kw):
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    solver = BatchedOCPSolver(N, S, 0.1, **(HELD if held else {}), **kw)
    if held:
        solver.set_rt_feasibility_tol(1e-2); solver.set_rt_position_row_cap(1e-5)
    if one_wave:
        solver.set_team_waves(1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    return solver, sb


def records(mpcs, recs, entries, **leg):
    """the re-plan records of tests/emu/emu_rollout.py small_batch for the streams of small_streams: a leg back over each stream's own via points"""
    from boundmpc_amd import stream as bstream
    from tests.emu import emu_rollout as er
    S = mpcs[0].nr_segs
    return np.stack([bstream.replan_record(S, entries, *er.leg_back(m, r, np.zeros((entries, 48)), S, **leg)) for m, r in zip(mpcs, recs)])


def snapshot(sb):
    return {k: getattr(sb, k).cpu().numpy().copy() for k in ARRAYS}


def history_rows(s):
    """what `hist` holds behind a tick, from the snapshot `s` of the batch"""
    from boundmpc_amd import stream as bstream
    SS = bstream.SS
    return np.concatenate([s["robot"], s["state"][:, [SS["PHI"], SS["ERRCNT"]]], s["iters"][:, None].astype(float), s["status"][:, None].astype(float), s["kkt"][:, None],
                           s["traj"][:, -4:]], axis=1)


def per_tick(sb, ticks, **kw):
    """`ticks` direct launches of the fused tick, read back after each: (hist rows [ticks][B][52], traj rows, snapshots); a stream the tick skipped
    (it had lost its plan before the tick) gets NaN rows"""
    import torch
    from boundmpc_amd import stream as bstream
    SS, rows, trajs, snaps = bstream.SS, [], [], []
    for _ in range(ticks):
        lost = sb.state[:, SS["ERRCNT"]].cpu().numpy() >= sb.N
        sb.tick(simulate=True, **kw)
        torch.cuda.synchronize()
        s = snapshot(sb)
        row, tr = history_rows(s), s["traj"].copy()
        row[lost] = np.nan; tr[lost] = np.nan
        rows.append(row); trajs.append(tr); snaps.append(s)
    return np.array(rows), np.array(trajs), snaps


def contract_loop(sb, ticks, records, tick_of, dist, want_tube=False, want_log=False, **kw):
    """The contract's loop on the batch `sb`: per tick one fused tick (on one wave per stream or on teams, as the batch's handle is set), then
    tube() and log() where wanted, bmpc_stream_disturb with the rows of the tick, bmpc_stream_update(set_goal, splice) with exactly the flags of the
    streams whose tick it is raised -- events for the streams that still run only.
    -> dict(hist [ticks][B][52], traj_hist, tube_hist [ticks][B][16], log_hist: whole rows [ticks][B][88 N + 4], ticks_run [B], replan_info [B]), NaN for
    the ticks a stream did not run, None for rows not wanted"""
    import torch
    from boundmpc_amd import stream as bstream
    SS, B = bstream.SS, sb.B
    r = dict(hist=np.full((ticks, B, 52), np.nan), traj_hist=np.full((ticks, B, sb.tr_len), np.nan), tube_hist=np.full((ticks, B, 16), np.nan) if want_tube else None,
             log_hist=np.full((ticks, B, bstream.log_len(sb.N)), np.nan) if want_log else None, ticks_run=np.zeros(B, dtype=int), replan_info=np.full(B, -1))
    sb._replan_buffer(records, None)
    stopped = np.zeros(B, dtype=bool)
    for t in range(ticks):
        stopped |= sb.state[:, SS["ERRCNT"]].cpu().numpy() >= sb.N
        sb.tick(simulate=True, **kw)
        tube, log = sb.tube() if want_tube else None, sb.log() if want_log else None
        torch.cuda.synchronize()
        s = snapshot(sb)
        live = ~stopped
        r["hist"][t, live], r["traj_hist"][t, live] = history_rows(s)[live], s["traj"][live]
        r["ticks_run"][live] = t + 1
        if want_tube:
            r["tube_hist"][t, live] = tube.cpu().numpy()[live]
        if want_log:
            r["log_hist"][t, live] = log.cpu().numpy()[live]
        d = dist[t].copy(); d[stopped] = 0.0
        sb.disturb(d)
        due = live & (tick_of == t)
        if due.any():
            flags = sb.replan[:, 0].clone()
            sb.replan[:, 0] = torch.where(torch.as_tensor(due, device=flags.device), flags, torch.zeros_like(flags))
            i = sb.update_device(sb.replan, set_goal=True, splice=True)
            torch.cuda.synchronize()
            r["replan_info"][due] = i.cpu().numpy()[due]
            sb.replan[:, 0] = torch.where(torch.as_tensor(due, device=flags.device), sb.replan[:, 0], flags)
    torch.cuda.synchronize()
    return r


def assert_equal(a, b, what, rows=None):
    for k in ARRAYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {k} differs"


def close(*pairs):
    for solver, sb in pairs:
        sb.close(); solver.close()
