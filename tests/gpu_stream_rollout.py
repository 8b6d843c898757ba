#!/usr/bin/env python3
"""Diagnostic (GPU; not a test, not part of bench.py): what a rollout saves over the per-tick loop.  The 256 closed-loop streams of BASELINE
configs[4] (workload.make_streams, N = 10, S = 4) over 130 ticks, HIP events around the WHOLE loop, a warm-up run of every variant first, then
`--reps` alternating repetitions, every run from the same initial state:
  (a) the shipped per-tick path: StreamBatch.closed_loop(graph=True) with the default wave choice (teams at B = 256) and with set_team_waves(1);
      beside the driver (which synchronises after every tick) the same launches enqueued back to back -- the faster of the two is what the rollout
      is held against;
  (b) tick 0 followed by rollout(129) (tick 0 on one wave, so that the final state can be compared bit for bit with the one-wave loop).
Modes: converged (tol 1e-8, dual state carried) and the held-barrier real-time mode bench.py reports for configs[4] (five iterations a tick);
then converged again at B = 1024 (the streams tiled four times).  Reported: wall time of the loop (median, min, max) and stream-ticks per
second; the final arrays of (b) against the one-wave loop (must be equal bit for bit) and against the team loop (the agreement tests/test_gpu_team.py
states for closed loops: robot records within 1e-7, trajectory records within 1e-6 -- counted per stream, loops of 130 ticks amplify a rounding
difference where a stream loses its plan).
Usage: python tests/gpu_stream_rollout.py [--out profiles/stream_rollout.txt] [--reps 5] [--ticks 130]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")


def make(mode, mpcs, recs, one_wave):
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    if mode == "held":
        solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-3, max_iter=30, fixed_barrier="auto", bound_margin=2e-3)
        solver.set_rt_feasibility_tol(1e-2); solver.set_rt_position_row_cap(1e-5)
    else:
        solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-8, mu_warm=1e-2, max_iter=100, stall_window=16)      # the handle of bench_stream.py's converged mode
        solver.set_restoration(cap=24)
    if one_wave:
        solver.set_team_waves(1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    return solver, sb


def run_mode(mode, mpcs, recs, ticks, reps, say):
    import torch
    B = len(mpcs)
    kw = dict(cap=5, accept_capped=True) if mode == "held" else dict(cap=0, accept_capped=False)
    tick_kw = dict(max_iter=kw["cap"], warm_dual=True, accept_capped=kw["accept_capped"])
    batches = {"team": make(mode, mpcs, recs, False), "one wave": make(mode, mpcs, recs, True), "rollout": make(mode, mpcs, recs, True)}
    init = {k: {a: getattr(sb, a).clone() for a in ARRAYS} for k, (_, sb) in batches.items()}
    for k, (_, sb) in batches.items():      # (p, x0, x, g come from torch.empty: zeroed, so that every run starts from the same bytes)
        for a in ("p", "x0", "x", "g"):
            init[k][a].zero_()

    def reset(k):
        for a in ARRAYS:
            getattr(batches[k][1], a).copy_(init[k][a])

    def driver(k):
        for _ in batches[k][1].closed_loop(ticks, first_cap=100, warm=True, graph=True, **kw):
            pass

    def back_to_back(k):
        sb = batches[k][1]
        sb.tick(max_iter=100, warm_dual=True, simulate=True)
        for _ in range(ticks - 1):
            sb.tick_graph(simulate=True, **tick_kw)

    def rollout(k):
        sb = batches[k][1]
        sb.tick(max_iter=100, warm_dual=True, simulate=True)
        return sb.rollout(ticks - 1, **tick_kw)

    variants = [("default waves, closed_loop driver", "team", driver), ("default waves, back to back", "team", back_to_back), ("one wave, closed_loop driver", "one wave", driver),
                ("one wave, back to back", "one wave", back_to_back), ("rollout", "rollout", rollout)]
    ms = {name: [] for name, _, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    final, ticks_run = {}, None
    with torch.cuda.stream(torch.cuda.Stream()):
        for rep in range(reps + 1):      # rep 0: warm-up (graphs captured, code objects loaded, workspace allocated)
            for name, k, fn in variants:
                reset(k); torch.cuda.synchronize()
                ev[0].record()
                out = fn(k)
                ev[1].record(); ev[1].synchronize()
                if rep:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
                final[name] = {a: getattr(batches[k][1], a).cpu().numpy().copy() for a in ARRAYS}
                if out is not None:
                    ticks_run = out["ticks_run"].cpu().numpy() + 1
    say(f"---- {mode}, B = {B} streams, {ticks} ticks, {reps} alternating repetitions ----")
    med = {}
    for name, _, _ in variants:
        v = np.array(ms[name]); med[name] = float(np.median(v))
        say(f"{name:36s} loop {np.median(v):9.2f} ms  (min {v.min():9.2f}, max {v.max():9.2f}, spread {v.max() - v.min():7.2f})  "
            f"{B * ticks / np.median(v) * 1e3:12.0f} stream-ticks/s   runs: {' '.join('%.2f' % x for x in v)}")
    best = min((n for n in med if n != "rollout"), key=med.get)
    spread = max(ms[best]) - min(ms[best])
    say(f"fastest per-tick loop: {best} ({med[best]:.2f} ms, run-to-run spread {spread:.2f} ms); rollout {med['rollout']:.2f} ms = {med['rollout'] / med[best]:.3f} of it; "
        f"gain {med[best] - med['rollout']:.2f} ms {'EXCEEDS' if med[best] - med['rollout'] > spread else 'DOES NOT EXCEED'} the spread")
    lost = int((final["rollout"]["status"] == 3).sum())
    say(f"streams that ran all ticks {int((ticks_run == ticks).sum())} of {B}, lost their plan {lost}; ticks run in all {int(ticks_run.sum())}")
    same = all(np.array_equal(final["rollout"][a], final["one wave, back to back"][a], equal_nan=True) for a in ARRAYS)
    same_drv = all(np.array_equal(final["one wave, closed_loop driver"][a], final["one wave, back to back"][a], equal_nan=True) for a in ARRAYS)
    say(f"final arrays, rollout against the one-wave loop: {'EQUAL bit for bit' if same else 'DIFFERENT'} ({', '.join(ARRAYS)}); driver against back to back: "
        f"{'equal' if same_drv else 'DIFFERENT'}")
    dr = np.abs(final["rollout"]["robot"] - final["default waves, back to back"]["robot"]).max(axis=1)
    dt = np.nanmax(np.abs(final["rollout"]["traj"] - final["default waves, back to back"]["traj"]), axis=1)
    say(f"final arrays, rollout against the default-waves loop (%d waves per stream): robot records within 1e-7 on {int((dr <= 1e-7).sum())} of {B} streams (largest {dr.max():.3e}), trajectory "
        f"records within 1e-6 on {int((dt <= 1e-6).sum())} of {B} (largest {dt.max():.3e})" % batches["team"][0].team_info(B)["waves"])
    for solver, sb in batches.values():
        sb.close(); solver.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_rollout.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=130)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    from boundmpc_amd import build, workload
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    mpcs, recs = workload.make_streams(args.batch, seed=3)
    say(f"rollout against the per-tick loop, N = 10, S = 4, source hash {build.source_hash()}; HIP events around the whole loop")
    ok = run_mode("converged", mpcs, recs, args.ticks, args.reps, say)
    ok = run_mode("held", mpcs, recs, args.ticks, args.reps, say) and ok
    ok = run_mode("converged", mpcs * 4, np.concatenate([recs] * 4), args.ticks, args.reps, say) and ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
