"""Diagnostic (GPU): what the plant level costs inside a rollout and what the launch saves against the per-tick host loop it replaces.  The workload of
bench_stream.py's held mode (BASELINE configs[4]: N = 10, S = 4, tick 0 solved out, then five iterations a tick under the real-time rule), 256 streams, the
variants alternating inside one process, all on this tree's library, medians of 7:
  (i)   cost of the level: bmpc_stream_rollout_plant with an IDENTITY table against bmpc_stream_rollout_tuned on identical arguments (a table of NaN settings,
        legs = 1: a re-plan with splice behind tick 64 of every stream, tracking record on), 129 ticks, on one wave per stream and on teams of four, HIP
        events around the launch; the final arrays compared bit for bit.  The sweeps kernels are the parent's but for the operand offset of the rollout
        arguments (profiles/stream_rollout_plant_resources.txt): the baseline in the same build.
  (ii)  what the launch saves: the plant entry with a non-identity table (rows cycling: gain 0.9 / LAG 0.5 / a clip at 2 rad/s^3 / DELAY 1) against the loop
        {tick(); plant_step(tick t)} of 129 ticks on one wave per stream, enqueued without a host read in between -- the cheapest form of the loop; a loop
        that draws its deviation on the host (read the robot records back, disturb()) adds a synchronisation per tick --; wall time box to box
        (synchronised at both ends); robot records, plant state and plant record compared.
profiles/stream_rollout_plant.txt quotes the output.
Usage: python tests/gpu_stream_rollout_plant.py [--reps 7] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj", "path")


def make(mpcs, recs):
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-3, max_iter=30, fixed_barrier="auto", bound_margin=2e-3)
    solver.set_rt_feasibility_tol(1e-2); solver.set_rt_position_row_cap(1e-5)
    solver.set_team_waves(1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    return solver, sb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ticks", type=int, default=130)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import torch
    from boundmpc_amd import build, stream as bstream, workload
    from tests.rollout_contract import records as leg_records
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    B, n = args.batch, args.ticks - 1
    tick_kw = dict(max_iter=5, warm_dual=True, accept_capped=True)
    say(f"plants inside a rollout: held mode, N = 10, S = 4, behind a solved-out tick 0, {n} ticks, {args.reps} alternating repetitions, source hash {build.source_hash()}")
    mpcs, recs = workload.make_streams(B, seed=3)
    solver, sb = make(mpcs, recs)
    back, at = leg_records(mpcs, recs, sb.entries), np.full(B, 64)
    sb.tick(max_iter=100, warm_dual=True, simulate=True)
    torch.cuda.synchronize()
    init = {a: getattr(sb, a).clone() for a in ARRAYS}
    dev = sb.path.device

    def restore():
        for a in ARRAYS:
            getattr(sb, a).copy_(init[a])
        sb.plant_reset()
        torch.cuda.synchronize()

    def final():
        torch.cuda.synchronize()
        return {a: getattr(sb, a).cpu().numpy().copy() for a in ARRAYS}

    # ---- (i) cost of the level ----
    say(f"(i) an identity plant table against the sweeps entry on identical arguments: B = {B} benchmark streams, a table of NaN settings, legs = 1 (a re-plan with splice behind "
        f"tick 64 of every stream), track=True; HIP events around the launch")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    nan = torch.full((B, bstream.TUNE["LEN"]), float("nan"), dtype=torch.float64, device=dev)
    ident = torch.as_tensor(np.tile(bstream.plant_identity(), (B, 1)), device=dev)
    legs = dict(legs=back[:, None], leg_tick=at[:, None], tune=nan)
    for waves in (1, 4):
        variants = [("sweeps entry  rollout(legs=, tune=NaN)", legs), ("plant entry   rollout(legs=, tune=NaN, plant=identity)", dict(legs, plant=ident, want_plant_rec=True)),
                    ("sweeps entry  again (the spread of its own runs)", legs)]
        ms, fin, outs = [[] for _ in variants], [None] * 3, [None] * 3
        for rep in range(args.reps + 1):      # rep 0: warm-up
            for v, (_, kw) in enumerate(variants):
                restore()
                ev[0].record()
                out = sb.rollout(n, track=True, waves=waves, **kw, **tick_kw)
                ev[1].record(); ev[1].synchronize()
                if rep:
                    ms[v].append(ev[0].elapsed_time(ev[1]))
                fin[v], outs[v] = final(), {k: t.cpu().numpy() for k, t in out.items()}
        med = [float(np.median(m)) for m in ms]
        for v, (name, _) in enumerate(variants):
            x = np.array(ms[v])
            say(f"  waves {waves}  {name:56s} median {med[v]:8.3f} ms  (min {x.min():8.3f}, max {x.max():8.3f}, spread {x.max() - x.min():6.3f} = {(x.max() - x.min()) / med[v] * 100:.2f} %)   "
                f"runs: {' '.join('%.3f' % y for y in x)}")
        pooled = np.array(ms[0] + ms[2])
        say(f"  waves {waves}  plant / sweeps = {med[1] / med[0]:.4f} ({med[1] - med[0]:+.3f} ms = {(med[1] - med[0]) / n * 1e3:+.2f} us a tick); the sweeps entry against itself "
            f"{med[2] / med[0]:.4f}; spread of the sweeps entry's {len(pooled)} runs {(pooled.max() - pooled.min()) / np.median(pooled) * 100:.2f} % of their median "
            f"[{pooled.min():.3f}, {pooled.max():.3f}]; the plant median lies {'INSIDE' if pooled.min() <= med[1] <= pooled.max() else 'OUTSIDE'} it")
        eq = all(np.array_equal(fin[0][a], fin[1][a], equal_nan=True) for a in ARRAYS) and all(np.array_equal(outs[0][k], outs[1][k], equal_nan=True)
                                                                                               for k in ("hist", "ticks_run", "track", "replan_info", "legs_done", "leg_fired"))
        say(f"  waves {waves}  final arrays, path tables, hist, ticks_run, track, replan_info, legs_done, leg_fired: {'EQUAL bit for bit' if eq else 'DIFFERENT'}; plant_info all 0: "
            f"{bool((outs[1]['plant_info'] == 0).all())}; plant steps {int(outs[1]['plant_rec'][:, 0].sum())} of {int(outs[1]['ticks_run'].sum())} stream-ticks")

    # ---- (ii) the launch against the per-tick loop ----
    rows = bstream.plant_table(4, gain=[[0.9] * 7, [np.nan] * 7, [np.nan] * 7, [np.nan] * 7], lag=[np.nan, 0.5, np.nan, np.nan], sat=[np.nan, np.nan, 2.0, np.nan],
                               delay=[np.nan, np.nan, np.nan, 1.0])
    table = torch.as_tensor(rows[np.arange(B) % 4], device=dev)
    say(f"(ii) a non-identity table (rows cycling: gain 0.9 / LAG 0.5 / a clip at 2 rad/s^3 / DELAY 1): ONE launch rollout(plant=) of {n} ticks against the loop "
        f"{{tick(); plant_step(tick t)}} of {n} ticks, no host read in between; one wave per stream; wall time box to box")
    wall, fin, st, rec = [[], []], [None, None], [None, None], [None, None]
    for rep in range(args.reps + 1):
        for v in range(2):
            restore()
            t0 = time.perf_counter()
            if v == 0:
                out = sb.rollout(n, plant=table, want_plant_rec=True, waves=1, **tick_kw)
            else:
                for t in range(n):
                    sb.tick(simulate=True, **tick_kw)
                    sb.plant_step(table, tick=t)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep:
                wall[v].append((t1 - t0) * 1e3)
            fin[v], st[v] = final(), sb.plant_state.cpu().numpy().copy()
            rec[v] = (out["plant_rec"] if v == 0 else sb.plant_rec).cpu().numpy().copy()
    med = [float(np.median(w)) for w in wall]
    for v, name in enumerate((f"ONE launch    rollout(plant=) of {B} streams", f"{n} x 2 launches  tick(); plant_step()")):
        x = np.array(wall[v])
        say(f"  {name:48s} median {med[v]:8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f})   runs: {' '.join('%.2f' % y for y in x)}")
    dev_rb = float(np.nanmax(np.abs(fin[0]["robot"] - fin[1]["robot"])))
    eq = all(np.array_equal(fin[0][a], fin[1][a], equal_nan=True) for a in ARRAYS) and np.array_equal(st[0], st[1], equal_nan=True) and np.array_equal(rec[0], rec[1], equal_nan=True)
    say(f"  loop / one launch = {med[1] / med[0]:.3f}; final arrays, plant state and plant record: {'EQUAL bit for bit' if eq else 'DIFFERENT'} (largest deviation of the robot records "
        f"{dev_rb:.2e}); streams that ran every tick {int((out['ticks_run'] == n).sum())} of {B}; ticks with a clip {int(rec[0][:, 1].sum())}; largest |u - c| {np.nanmax(rec[0][:, 2]):.3f} rad/s^3")
    sb.close(); solver.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
