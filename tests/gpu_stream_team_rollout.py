#!/usr/bin/env python3
"""Diagnostic (GPU; not a test, not part of bench.py): what the rollout gains on TEAMS.  The closed-loop streams of BASELINE configs[4]
(workload.make_streams, N = 10, S = 4) over 130 ticks -- tick 0 followed by rollout(129) --, HIP events around the WHOLE loop, a warm-up run of every
variant first, then `--reps` alternating repetitions inside one process, every run from the same initial state:
  team rollout       tick 0 on teams, rollout(129, waves=4)
  one-wave rollout   tick 0 on one wave, rollout(129, waves=1)
  team loop          StreamBatch.closed_loop(graph=True) with the default wave choice (teams at these batch sizes)
Modes: the held-barrier real-time mode bench.py reports for configs[4] (five iterations a tick) and converged (tol 1e-8, dual state carried), at
B = 256; then held again at B = 16 and B = 1 (the reference's own single loop).  Reported: wall time of the loop (median, min, max, spread), the
streams that kept their plan in every variant, and how far the team rollout's final robot records are from the team loop's (the tick body is the team
tick's: bit-equal is expected).  The numbers to hold the team rollout against are the two variants measured beside it.
Usage: python tests/gpu_stream_team_rollout.py [--out profiles/stream_team_rollout.txt] [--reps 5] [--ticks 130]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.gpu_stream_rollout import ARRAYS, make      # noqa: E402  (the handles of the two modes)


def run_mode(mode, mpcs, recs, ticks, reps, say):
    import torch
    from boundmpc_amd import stream as bstream
    B = len(mpcs)
    kw = dict(cap=5, accept_capped=True) if mode == "held" else dict(cap=0, accept_capped=False)
    tick_kw = dict(max_iter=kw["cap"], warm_dual=True, accept_capped=kw["accept_capped"])
    batches = {"team rollout": make(mode, mpcs, recs, False), "one-wave rollout": make(mode, mpcs, recs, True), "team loop": make(mode, mpcs, recs, False)}
    init = {k: {a: getattr(sb, a).clone() for a in ARRAYS} for k, (_, sb) in batches.items()}
    for k in batches:      # (p, x0, x, g come from torch.empty: zeroed, so that every run starts from the same bytes)
        for a in ("p", "x0", "x", "g"):
            init[k][a].zero_()

    def reset(k):
        for a in ARRAYS:
            getattr(batches[k][1], a).copy_(init[k][a])

    def rollout(k, waves):
        sb = batches[k][1]
        sb.tick(max_iter=100, warm_dual=True, simulate=True)
        sb.rollout(ticks - 1, waves=waves, **tick_kw)

    def loop(k):
        for _ in batches[k][1].closed_loop(ticks, first_cap=100, warm=True, graph=True, **kw):
            pass

    variants = [("team rollout", lambda: rollout("team rollout", 4)), ("one-wave rollout", lambda: rollout("one-wave rollout", 1)), ("team loop", lambda: loop("team loop"))]
    assert batches["team loop"][0].team_info(B)["waves"] == 4
    ms = {name: [] for name, _ in variants}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    final = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        for rep in range(reps + 1):      # rep 0: warm-up (graphs captured, code objects loaded, workspace allocated)
            for name, fn in variants:
                reset(name); torch.cuda.synchronize()
                ev[0].record()
                fn()
                ev[1].record(); ev[1].synchronize()
                if rep:
                    ms[name].append(ev[0].elapsed_time(ev[1]))
                final[name] = {a: getattr(batches[name][1], a).cpu().numpy().copy() for a in ARRAYS}
    say(f"---- {mode}, B = {B} streams, {ticks} ticks, {reps} alternating repetitions ----")
    med = {}
    for name, _ in variants:
        v = np.array(ms[name]); med[name] = float(np.median(v))
        kept = int((final[name]["state"][:, bstream.SS["ERRCNT"]] < 10).sum())
        say(f"{name:18s} loop {np.median(v):9.2f} ms  (min {v.min():9.2f}, max {v.max():9.2f}, spread {v.max() - v.min():7.2f})  kept their plan {kept:3d} of {B}   "
            f"runs: {' '.join('%.2f' % x for x in v)}")
    t, o, l = med["team rollout"], med["one-wave rollout"], med["team loop"]
    say(f"team rollout = {t / o:.3f} of the one-wave rollout, {t / l:.3f} of the team loop: {'FASTER than both' if t < o and t < l else 'NOT faster than both'}")
    same = all(np.array_equal(final["team rollout"][a], final["team loop"][a], equal_nan=True) for a in ARRAYS)
    dr = np.abs(final["team rollout"]["robot"] - final["team loop"]["robot"]).max()
    d1 = np.abs(final["team rollout"]["robot"] - final["one-wave rollout"]["robot"]).max(axis=1)
    say(f"final arrays, team rollout against the team loop: {'EQUAL bit for bit' if same else 'DIFFERENT'}; largest robot-record difference {dr:.3e}")
    say(f"final robot records, team rollout against the one-wave rollout: within 1e-7 on {int((d1 <= 1e-7).sum())} of {B} streams (largest {d1.max():.3e})")
    for solver, sb in batches.values():
        sb.close(); solver.close()
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_team_rollout.txt"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=130)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    from boundmpc_amd import build, workload
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    mpcs, recs = workload.make_streams(args.batch, seed=3)
    say(f"team rollout against the one-wave rollout and the team loop, N = 10, S = 4, source hash {build.source_hash()}; HIP events around the whole loop")
    ok = run_mode("held", mpcs, recs, args.ticks, args.reps, say)
    ok = run_mode("converged", mpcs, recs, args.ticks, args.reps, say) and ok
    for B in (16, 1):
        if B < args.batch:
            ok = run_mode("held", mpcs[:B], recs[:B], args.ticks, args.reps, say) and ok
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
