"""What the GPU tests of the rollouts (tests/test_gpu_stream_*rollout*.py, tests/test_gpu_stream_tube.py) and their diagnostic scripts share: small
batches with a twin, snapshots of the tick arrays, the contract's loop on a batch -- per tick {fused tick, [plant step], [tube], [log], disturb, update of
the records due: scheduled, or the heads of the queues} with the rollout's stop rules -- that is the exact checker of every rollout variant (on one wave
per stream or, with set_team_waves(4), on teams), and the direct call of any of the seven entries of the C ABI (raw_rollout).  The CPU twin of the loop, on the g++ build of the same kernel text: tests/emu/emu_rollout.py contract_loop.  No test in here."""
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


def contract_loop(sb, ticks, records=None, tick_of=None, dist=None, want_tube=False, want_log=False, queue=None, leg_tick=None, leg_on=None, leg_tol=None, plant=None, **kw):
    """The contract's loop on the batch `sb`: per tick one fused tick (on one wave per stream or on teams, as the batch's handle is set), then
    plant_step(tick t) with a plant table [B][20] (the drives start where the launch starts them: plant_reset ahead of the first tick), then tube() and
    log() where wanted, bmpc_stream_disturb with the rows of the tick, then bmpc_stream_update(set_goal, splice) with exactly the flags of the streams
    raised whose record is due -- events for the streams that still run only.  The record due: of `records` [B][len] the one whose tick tick_of[b] it
    is; of `queue` [B][K][len] (a copy is advanced as the device's queue buffer is) the HEAD record when the host, which reads the state rows, finds one
    of its conditions to hold (tests/emu/emu_rollout.py due; leg_tick [B][K], leg_on and leg_tol [B][K] or None: no condition but the tick, tolerance 0).
    -> dict(hist [ticks][B][52], traj_hist, tube_hist [ticks][B][16], log_hist: whole rows [ticks][B][88 N + 4], ticks_run [B], replan_info [B] or
    [B][K], with a queue legs_done [B], leg_fired, leg_why [B][K] and queue, with a plant table plant_state and plant_rec), NaN for the ticks a stream did
    not run, None for rows not wanted"""
    import torch
    from boundmpc_amd import stream as bstream
    from tests.emu.emu_rollout import due as due_of
    SS, B = bstream.SS, sb.B
    r = dict(hist=np.full((ticks, B, 52), np.nan), traj_hist=np.full((ticks, B, sb.tr_len), np.nan), tube_hist=np.full((ticks, B, 16), np.nan) if want_tube else None,
             log_hist=np.full((ticks, B, bstream.log_len(sb.N)), np.nan) if want_log else None, ticks_run=np.zeros(B, dtype=int), replan_info=np.full(B, -1))
    if queue is not None:
        K = queue.shape[1]
        lo, tol = (np.zeros((B, K), dtype=dt) if a is None else np.asarray(a) for a, dt in ((leg_on, int), (leg_tol, float)))
        r.update(queue=queue.copy(), legs_done=np.zeros(B, dtype=int), leg_fired=np.full((B, K), -1), leg_why=np.zeros((B, K), dtype=int), replan_info=np.full((B, K), -1))
    elif records is not None:
        sb._replan_buffer(records, None)
    if plant is not None:
        sb.plant_reset()
    stopped = np.zeros(B, dtype=bool)
    for t in range(ticks):
        stopped |= sb.state[:, SS["ERRCNT"]].cpu().numpy() >= sb.N
        sb.tick(simulate=True, **kw)
        info = sb.plant_step(plant, tick=t) if plant is not None else None
        tube, log = sb.tube() if want_tube else None, sb.log() if want_log else None
        torch.cuda.synchronize()
        assert info is None or not info.any()
        s = snapshot(sb)
        live = ~stopped
        r["hist"][t, live], r["traj_hist"][t, live] = history_rows(s)[live], s["traj"][live]
        r["ticks_run"][live] = t + 1
        if want_tube:
            r["tube_hist"][t, live] = tube.cpu().numpy()[live]
        if want_log:
            r["log_hist"][t, live] = log.cpu().numpy()[live]
        if dist is not None:
            d = dist[t].copy(); d[stopped] = 0.0
            sb.disturb(d)
        if queue is not None:
            head = np.minimum(r["legs_done"], K - 1)
            why = np.array([due_of(sb.N, s["state"][b], t, leg_tick[b, head[b]], lo[b, head[b]], tol[b, head[b]]) if live[b] and r["legs_done"][b] < K else 0 for b in range(B)])
            if why.any():
                recs = r["queue"][np.arange(B), head].copy()
                recs[why == 0, 0] = 0.0
                i = sb.update_device(recs, set_goal=True, splice=True)
                torch.cuda.synchronize()
                after = sb.replan.cpu().numpy()
                for b in np.nonzero(why)[0]:
                    r["queue"][b, head[b]] = after[b]
                    r["replan_info"][b, head[b]], r["leg_fired"][b, head[b]], r["leg_why"][b, head[b]] = int(i[b]), t, why[b]
                    r["legs_done"][b] += 1
            continue
        due = live & (tick_of == t) if records is not None else np.zeros(B, dtype=bool)
        if due.any():
            flags = sb.replan[:, 0].clone()
            sb.replan[:, 0] = torch.where(torch.as_tensor(due, device=flags.device), flags, torch.zeros_like(flags))
            i = sb.update_device(sb.replan, set_goal=True, splice=True)
            torch.cuda.synchronize()
            r["replan_info"][due] = i.cpu().numpy()[due]
            sb.replan[:, 0] = torch.where(torch.as_tensor(due, device=flags.device), sb.replan[:, 0], flags)
    torch.cuda.synchronize()
    if plant is not None:
        r["plant_state"], r["plant_rec"] = sb.plant_state.cpu().numpy(), sb.plant_rec.cpu().numpy()
    return r


# the arguments of the rollout entries of the C ABI behind the tick arrays, by group: entry k takes the first k groups (the queue entries, 4 to 6, take no replan_tick)
RAW_HEAD = ("handle", "B", "ticks", "path", "entries", "state", "robot", "p", "x0", "dual", "max_iter", "x", "g", "iters", "status", "kkt", "traj", "flags", "goal_tol", "hist",
            "traj_hist", "ticks_run")
RAW_GROUPS = (("replan", "replan_tick", "replan_info", "update_flags", "disturb"), ("tube_hist", "audit", "audit_tol"), ("log_hist", "log_stages", "track"),
              ("legs", "leg_tick", "leg_on", "leg_tol", "legs_done", "leg_fired", "leg_why"), ("tune", "tune_info", "tune_used"), ("plant", "plant_state", "plant_info", "plant_rec"))
RAW_INT32 = ("replan_tick", "leg_tick", "leg_on")


def raw_rollout(solver, sb, entry, tensors=None, outputs=False, waves=None, **over):
    """The C ABI entry number `entry` called directly with the batch's own tensors (or `tensors`: ARRAYS + path, of `B` streams), chosen arguments replaced:
    `over` names arguments of the entry (RAW_HEAD, RAW_GROUPS; an array is put on the device, a tensor taken as it is, None is NULL).  What is not named:
    ticks 2, max_iter 0, flags 1, goal_tol 0, update_flags 3, audit_tol 1e-6, log_stages 1, legs = the K of a queue `replan` [B][K][len] (1 without one),
    every other pointer NULL -- or, with outputs=True, every output array of the entry, filled with -7.  waves: set for the call, the former setting put
    back.  -> (the return code, dict of what was passed by name: the device tensors live on in it)"""
    import torch
    from boundmpc_amd.solver import _ptr
    from boundmpc_amd.stream import ROLLOUT_ENTRIES as ENTRIES
    dev = sb.path.device
    names = RAW_HEAD + tuple(n for g in RAW_GROUPS[:entry] for n in g if not (n == "replan_tick" and entry >= 4))
    a = dict(handle=solver._h, B=sb.B, ticks=2, entries=sb.entries, max_iter=0, flags=1, goal_tol=0.0, update_flags=3, audit_tol=1e-6, log_stages=1, legs=1)
    a.update({k: getattr(sb, k) for k in ARRAYS + ("path",)} if tensors is None else tensors)
    for k, v in over.items():
        assert k in names, f"{ENTRIES[entry]} has no argument {k}"
        a[k] = v if v is None or np.isscalar(v) or torch.is_tensor(v) else torch.as_tensor(np.ascontiguousarray(v), device=dev).to(torch.int32 if k in RAW_INT32 else torch.float64).contiguous()
    if a.get("replan") is not None and entry >= 4 and "legs" not in over:
        a["legs"] = a["replan"].shape[1]
    if outputs:
        n, B, K = a["ticks"], a["B"], (max(a["legs"], 1),) if entry >= 4 else ()
        shapes = dict(hist=(n, B, 52), traj_hist=(n, B, sb.tr_len), ticks_run=(B,), replan_info=(B,) + K, tube_hist=(n, B, 16), audit=(B, 12), log_hist=(n, B, 88 * a["log_stages"] + 4),
                      track=(B, 12), legs_done=(B,), leg_fired=(B,) + K, leg_why=(B,) + K, tune_info=(B,), tune_used=(B, 16), plant_info=(B,), plant_rec=(B, 8))
        ints = ("ticks_run", "replan_info", "legs_done", "leg_fired", "leg_why", "tune_info", "plant_info")
        for k, shape in shapes.items():
            if k in names and k not in over:
                a[k] = torch.full(shape, -7, dtype=torch.int32 if k in ints else torch.float64, device=dev)
    former = solver.rollout_waves
    if waves is not None:
        solver.set_rollout_waves(waves)
    rc = getattr(solver._lib, ENTRIES[entry])(*[_ptr(a.get(k)) if torch.is_tensor(a.get(k)) else a.get(k) for k in names], None)
    solver.set_rollout_waves(former)
    return rc, a


def assert_equal(a, b, what, rows=None):
    for k in ARRAYS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert np.array_equal(x, y, equal_nan=True), f"{what}: {k} differs"


def close(*pairs):
    for solver, sb in pairs:
        sb.close(); solver.close()
