"""Diagnostic (GPU): what the observer level costs inside a rollout, what the launch saves against the per-tick host loop it replaces, and what the level exists
for.  The workload of bench_stream.py's held mode (BASELINE configs[4]: N = 10, S = 4, tick 0 solved out, then five iterations a tick under the real-time
rule), 256 streams, the variants alternating inside one process, all on this tree's library, medians of `--reps`:
  (i)   cost of the level: bmpc_stream_rollout_observer with an IDENTITY observer table against bmpc_stream_rollout_sensor on identical arguments (the arguments
        of tests/gpu_stream_rollout_sensor.py (i): identity sensor and plant tables, a table of NaN settings, legs = 1: a re-plan with splice behind tick 64 of
        every stream, tracking record on), 129 ticks, on one wave per stream and on teams of four, HIP events around the launch; the final arrays compared bit
        for bit.
  (ii)  what the launch saves: the observer entry with the non-identity sensor table of tests/gpu_stream_rollout_sensor.py (ii) (rows cycling: offsets with noise
        / a 16-bit encoder step / HOLD with noise / offsets) and an observer with gains 0.3 on q, dq and ddq and LEAD on the HOLD rows, against the loop
        {observe(tick t); tick(); unsense()} of 129 ticks on one wave per stream, enqueued without a host read in between; wall time box to box; robot records,
        the two states and the two records compared.
  (iii) the question the level exists for: on that sensor table, how many of the streams keep a plan for all ticks without an observer (the sensor's entry) and
        with the observer of (ii); the records of the two runs beside each other.
profiles/stream_rollout_observer.txt quotes the output of two runs.
Usage: python tests/gpu_stream_rollout_observer.py [--reps 5] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj", "path")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=130)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import torch
    from boundmpc_amd import build, stream as bstream, workload
    from tests.gpu_stream_rollout_plant import make
    from tests.rollout_contract import records as leg_records
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    B, n = args.batch, args.ticks - 1
    tick_kw = dict(max_iter=5, warm_dual=True, accept_capped=True)
    say(f"observers inside a rollout: held mode, N = 10, S = 4, behind a solved-out tick 0, {n} ticks, {args.reps} alternating repetitions, source hash {build.source_hash()}")
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
        sb.plant_reset(); sb.sensor_reset(); sb.observer_reset()
        torch.cuda.synchronize()

    def final():
        torch.cuda.synchronize()
        return {a: getattr(sb, a).cpu().numpy().copy() for a in ARRAYS}

    # ---- (i) cost of the level ----
    say(f"(i) an identity observer table against the sensors' entry on identical arguments: B = {B} benchmark streams, identity sensor and plant tables, a table of NaN settings, "
        f"legs = 1 (a re-plan with splice behind tick 64 of every stream), track=True; HIP events around the launch")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    nan = torch.full((B, bstream.TUNE["LEN"]), float("nan"), dtype=torch.float64, device=dev)
    pident = torch.as_tensor(np.tile(bstream.plant_identity(), (B, 1)), device=dev)
    sident = torch.zeros((B, bstream.SENSOR["LEN"]), dtype=torch.float64, device=dev)
    oident = torch.as_tensor(np.tile([1.0, 1.0, 1.0, 0.0, np.inf, 0.0, 0.0, 0.0], (B, 1)), device=dev)
    base = dict(legs=back[:, None], leg_tick=at[:, None], tune=nan, plant=pident, want_plant_rec=True, sensor=sident, want_sensor_rec=True)
    for waves in (1, 4):
        variants = [("sensors' entry  rollout(..., sensor=identity)", base), ("observer entry  rollout(..., observer=identity)", dict(base, observer=oident, want_observer_rec=True)),
                    ("sensors' entry  again (the spread of its own runs)", base)]
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
        say(f"  waves {waves}  observer / sensors = {med[1] / med[0]:.4f} ({med[1] - med[0]:+.3f} ms = {(med[1] - med[0]) / n * 1e3:+.2f} us a tick); the sensors' entry against itself "
            f"{med[2] / med[0]:.4f}; spread of the sensors' entry's {len(pooled)} runs {(pooled.max() - pooled.min()) / np.median(pooled) * 100:.2f} % of their median "
            f"[{pooled.min():.3f}, {pooled.max():.3f}]; the observer median lies {'INSIDE' if pooled.min() <= med[1] <= pooled.max() else 'OUTSIDE'} it")
        eq = all(np.array_equal(fin[0][a], fin[1][a], equal_nan=True) for a in ARRAYS) and all(np.array_equal(outs[0][k], outs[1][k], equal_nan=True)
                                                                                               for k in ("hist", "ticks_run", "track", "replan_info", "legs_done", "leg_fired", "plant_rec", "sensor_rec"))
        say(f"  waves {waves}  final arrays, path tables, hist, ticks_run, track, replan_info, legs_done, leg_fired, plant_rec, sensor_rec: {'EQUAL bit for bit' if eq else 'DIFFERENT'}; "
            f"observer_info all 0: {bool((outs[1]['observer_info'] == 0).all())}; estimates {int(outs[1]['observer_rec'][:, 0].sum())} of {int(outs[1]['ticks_run'].sum())} stream-ticks")

    # ---- (ii) the launch against the per-tick loop ----
    rows = bstream.sensor_table(4, bias=[[1e-3] * 7, [np.nan] * 7, [np.nan] * 7, [5e-4] * 7], nq=[1e-4, np.nan, 1e-4, np.nan], res=[np.nan, 2 * np.pi / 2 ** 16, np.nan, np.nan],
                                hold=[np.nan, np.nan, 1.0, np.nan])
    orows = bstream.observer_table(4, lq=0.3, ldq=0.3, lddq=0.3, lead=[np.nan, np.nan, 1.0, np.nan])
    table = torch.as_tensor(rows[np.arange(B) % 4], device=dev)
    otable = torch.as_tensor(orows[np.arange(B) % 4], device=dev)
    noise = torch.as_tensor(np.random.default_rng(5).normal(size=(n, B, 21)), device=dev)
    say(f"(ii) the sensors' non-identity table (rows cycling: offsets with noise / a 16-bit encoder step / HOLD with noise / offsets) and an observer with gains 0.3 on q, dq, ddq and LEAD "
        f"on the HOLD rows: ONE launch rollout(sensor=, observer=) of {n} ticks against the loop {{observe(tick t); tick(); unsense()}} of {n} ticks, no host read in between; one wave "
        f"per stream; wall time box to box")
    wall, fin, st, rec = [[], []], [None, None], [None, None], [None, None]
    for rep in range(args.reps + 1):
        for v in range(2):
            restore()
            t0 = time.perf_counter()
            if v == 0:
                out = sb.rollout(n, sensor=table, sensor_noise=noise, want_sensor_rec=True, observer=otable, want_observer_rec=True, waves=1, **tick_kw)
            else:
                for t in range(n):
                    sb.observe(table, otable, noise[t], tick=t)
                    sb.tick(simulate=True, **tick_kw)
                    sb.unsense(table)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep:
                wall[v].append((t1 - t0) * 1e3)
            fin[v], st[v] = final(), (sb.sensor_state().cpu().numpy().copy(), sb.observer_state().cpu().numpy().copy())
            rec[v] = tuple(x.cpu().numpy().copy() for x in ((out["sensor_rec"], out["observer_rec"]) if v == 0 else (sb.sensor_rec, sb.observer_rec)))
    med = [float(np.median(w)) for w in wall]
    for v, name in enumerate((f"ONE launch    rollout(sensor=, observer=) of {B} streams", f"{n} x 3 launches  observe(); tick(); unsense()")):
        x = np.array(wall[v])
        say(f"  {name:56s} median {med[v]:8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f})   runs: {' '.join('%.2f' % y for y in x)}")
    dev_rb = float(np.nanmax(np.abs(fin[0]["robot"] - fin[1]["robot"])))
    with_ob = out["ticks_run"].cpu().numpy()
    ran = with_ob == n
    eq = all(np.array_equal(fin[0][a][ran], fin[1][a][ran], equal_nan=True) for a in ARRAYS) and all(np.array_equal(st[0][k][ran], st[1][k][ran], equal_nan=True) for k in (0, 1)) \
        and all(np.array_equal(rec[0][k][ran], rec[1][k][ran], equal_nan=True) for k in (0, 1))
    say(f"  loop / one launch = {med[1] / med[0]:.3f}; final arrays, sensor and observer states and records of the streams that ran every tick: {'EQUAL bit for bit' if eq else 'DIFFERENT'} "
        f"(largest deviation of the robot records {dev_rb:.2e}); streams that ran every tick {int(ran.sum())} of {B}")

    # ---- (iii) what the level is for ----
    restore()
    plain = sb.rollout(n, sensor=table, sensor_noise=noise, want_sensor_rec=True, waves=1, **tick_kw)
    torch.cuda.synchronize()
    without = plain["ticks_run"].cpu().numpy()
    srec, orec, srec0 = rec[0][0], rec[0][1], plain["sensor_rec"].cpu().numpy()
    say(f"(iii) streams of {B} that keep a plan for all {n} ticks on that sensor table: WITHOUT an observer {int((without == n).sum())}, WITH gains 0.3 and LEAD on the HOLD rows "
        f"{int(ran.sum())}; by row of the sensor table (offsets with noise / encoder step / HOLD with noise / offsets): without "
        f"{[int((without[np.arange(B) % 4 == k] == n).sum()) for k in range(4)]}, with {[int(ran[np.arange(B) % 4 == k].sum()) for k in range(4)]} of {B // 4} each")
    both = ran & (without == n)
    say(f"  over the {int(both.sum())} streams that ran every tick in both runs: largest |q_m - q| of the samples {np.nanmax(srec[both][:, 1]):.2e} rad with the observer, "
        f"{np.nanmax(srec0[both][:, 1]):.2e} without; largest |q_est - q| of the estimates {np.nanmax(orec[both][:, 2]):.2e} rad; rms of q_est - q {np.sqrt(orec[both][:, 7].sum() / (7 * n * both.sum())):.2e}, "
        f"of q_m - q {np.sqrt(srec[both][:, 6].sum() / (7 * n * both.sum())):.2e} with the observer and {np.sqrt(srec0[both][:, 6].sum() / (7 * n * both.sum())):.2e} without; "
        f"samples the gate rejected {int(orec[:, 1].sum())}")
    sb.close(); solver.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
