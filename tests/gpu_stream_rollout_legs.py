"""Diagnostic (GPU): what a mission inside a rollout costs and what it buys.  The workload of bench_stream.py's held mode (BASELINE configs[4]: 256
streams, N = 10, S = 4, tick 0 solved out, then five iterations a tick under the real-time rule), on one wave per stream and on teams of four, the
variants alternating inside one process, all on this tree's library, medians of 7:
  (i)  dormant cost: bmpc_stream_rollout_legs with legs = 1 against bmpc_stream_rollout_log on identical arguments (one re-plan with splice behind tick
       64 of every stream, tracking record on), 129 ticks, HIP events around the launch; the final arrays compared bit for bit.
  (ii) what the queue buys: a mission of three goal-triggered legs -- to the stream's first waypoint (re-planned ahead of the box), back to its start,
       to the waypoint again; every leg a straight path of two via points from where the plant is -- in ONE launch (two records AT_GOAL with the
       launch's goal_tol = GOAL, the last goal stops the stream) against the only alternative without it: three rollouts with goal_tol of at most CAP
       ticks, each followed by update_device(splice=True); then the same on a batch of the streams that reach every goal in both.  Wall time box to box (synchronised at both ends); leg_fired against the chain's ticks_run; the final arrays of the streams that fly all three legs in both compared bit for bit.
profiles/stream_rollout_legs.txt quotes the output.
Usage: python tests/gpu_stream_rollout_legs.py [--reps 7] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj", "path")
GOAL, CAP = 0.02, 150


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
    mpcs, recs = workload.make_streams(args.batch, seed=3)
    B, ticks = args.batch, args.ticks
    tick_kw = dict(max_iter=5, warm_dual=True, accept_capped=True)
    solver, sb = make(mpcs, recs)
    back = leg_records(mpcs, recs, sb.entries)
    sb.tick(max_iter=100, warm_dual=True, simulate=True)      # tick 0, solved out: every variant starts behind it
    torch.cuda.synchronize()
    init = {a: getattr(sb, a).clone() for a in ARRAYS}

    def short_legs(j):
        """[B][len]: a straight leg from the pose the splice writes to via point j of the stream's own path (0: its start, 1: its first waypoint)"""
        from tests.emu import emu_rollout as er
        out = []
        for m, r in zip(mpcs, recs):
            a = er.leg_back(m, r, np.zeros((sb.entries, 48)), sb.S)      # (its via points run from the end of the path back to the start)
            two = lambda lst: [lst[0], lst[len(lst) - 1 - j]]
            a = [two(a[0]), two(a[1]), [two(a[2][0]), two(a[2][1])], [two(a[3][0]), two(a[3][1])], a[4], a[5]] + [two(x) for x in a[6:11]] + a[11:]
            out.append(bstream.replan_record(sb.S, sb.entries, *a))
        return np.stack(out)

    def restore():
        for a in ARRAYS:
            getattr(sb, a).copy_(init[a])
        torch.cuda.synchronize()

    def final():
        torch.cuda.synchronize()
        return {a: getattr(sb, a).cpu().numpy().copy() for a in ARRAYS}
    same = lambda x, y: all(np.array_equal(x[a], y[a], equal_nan=True) for a in ARRAYS)
    say(f"missions inside a rollout: held mode, B = {B} streams, N = 10, S = 4, behind a solved-out tick 0, {args.reps} alternating repetitions, source hash {build.source_hash()}")

    # ---- (i) dormant cost ----
    n, at = ticks - 1, np.full(B, 64)
    say(f"(i) legs = 1 against the log entry on identical arguments: {n} ticks, a re-plan with splice behind tick 64 of every stream, track=True; HIP events around the launch")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for waves in (1, 4):
        variants = [("log entry   rollout(replan=, replan_tick=)", dict(replan=back, replan_tick=at)), ("legs entry  rollout(legs=, leg_tick=), legs = 1", dict(legs=back[:, None], leg_tick=at[:, None])),
                    ("log entry   again (the spread of its own runs)", dict(replan=back, replan_tick=at))]
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
            say(f"  waves {waves}  {name:50s} median {med[v]:8.3f} ms  (min {x.min():8.3f}, max {x.max():8.3f}, spread {x.max() - x.min():6.3f})   runs: {' '.join('%.3f' % y for y in x)}")
        pooled = np.array(ms[0] + ms[2])
        say(f"  waves {waves}  legs / log = {med[1] / med[0]:.4f} ({med[1] - med[0]:+.3f} ms = {(med[1] - med[0]) / n * 1e3:+.2f} us a tick); the log entry against itself {med[2] / med[0]:.4f}; "
            f"spread of the log entry's {len(pooled)} runs {(pooled.max() - pooled.min()) / np.median(pooled) * 100:.2f} % of their median")
        eq = same(fin[0], fin[1]) and all(np.array_equal(outs[0][k], outs[1][k], equal_nan=True) for k in ("hist", "ticks_run", "track")) \
            and np.array_equal(outs[0]["replan_info"], outs[1]["replan_info"][:, 0])
        say(f"  waves {waves}  final arrays, path tables, hist, ticks_run, track, replan_info: {'EQUAL bit for bit' if eq else 'DIFFERENT'}; records consumed {int(outs[1]['legs_done'].sum())} of {B}, "
            f"stream-ticks {int(outs[1]['ticks_run'].sum())}")

    # ---- (ii) one launch against the chain ----
    keep = None
    for part in range(2):      # every stream; then, on a batch of their own, the streams on which the two variants do the same work
        if part == 0:
            restore()
        else:
            idx = np.nonzero(keep)[0]
            if len(idx) == 0:
                break
            sb.close(); solver.close()
            mpcs, recs, B = [mpcs[i] for i in idx], recs[idx], len(idx)
            solver, sb = make(mpcs, recs)
            sb.tick(max_iter=100, warm_dual=True, simulate=True)
            torch.cuda.synchronize()
            say(f"(ii b) the same on a batch of those {B} streams alone: both variants run the same ticks of the same streams")
        to_start, to_waypoint = short_legs(0), short_legs(1)
        info = sb.update_device(to_waypoint, splice=True)      # leg A, ahead of the box: both variants start on it
        torch.cuda.synchronize()
        init = {a: getattr(sb, a).clone() for a in ARRAYS}
        goal_tol = GOAL
        say(f"(ii) three goal-triggered legs (waypoint 1, start, waypoint 1; phi_max of leg A {float(sb.state[:, bstream.SS['PHIMAX']].min()):.3f}..{float(sb.state[:, bstream.SS['PHIMAX']].max()):.3f}, "
            f"records refused {int((info != 0).sum())}): goal_tol {goal_tol}; the one launch has {3 * CAP} ticks, a link of the chain at most {CAP}; wall time box to box")
        queue = np.ascontiguousarray(np.stack([to_start, to_waypoint], axis=1))
        dev = sb.path.device      # (the records and trigger words wait on the device in both variants: no host copy inside the box)
        qdev, on = torch.as_tensor(queue, device=dev), torch.full((B, 2), bstream.LEG["AT_GOAL"], dtype=torch.int32, device=dev)
        links = [qdev[:, k].contiguous() for k in range(2)]
        for waves in (1, 4):
            wall, fin, res = [[], []], [None, None], [None, None]
            for rep in range(args.reps + 1):
                for v in range(2):
                    restore()
                    t0 = time.perf_counter()
                    if v == 0:
                        out = sb.rollout(3 * CAP, goal_tol=goal_tol, legs=qdev, leg_on=on, waves=waves, **tick_kw)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        got = {k: t.cpu().numpy() for k, t in out.items()}
                    else:
                        runs = []
                        for link in range(3):
                            out = sb.rollout(CAP, goal_tol=goal_tol, waves=waves, **tick_kw)
                            runs.append(out["ticks_run"])
                            if link < 2:
                                sb.update_device(links[link], splice=True)
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        got = {"runs": np.stack([r.cpu().numpy() for r in runs])}
                    if rep:
                        wall[v].append((t1 - t0) * 1e3)
                    fin[v], res[v] = final(), got
            med = [float(np.median(w)) for w in wall]
            for v, name in enumerate(("ONE launch  rollout(legs=, leg_on=AT_GOAL, goal_tol=)", "chain       3 x {rollout(goal_tol=), update_device(splice=True)}")):
                x = np.array(wall[v])
                say(f"  waves {waves}  {name:62s} median {med[v]:8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f})   runs: {' '.join('%.2f' % y for y in x)}")
            m, runs = res[0], res[1]["runs"]
            cum = np.cumsum(runs, axis=0)
            # streams on which the two mean the same: every goal reached inside its link, by the goal rule (a stream that misses one is re-planned by the chain
            # and not by the mission; one whose next leg is shorter than goal_tol stops behind the re-plan in the mission and flies a tick of it in the chain)
            both = (m["legs_done"] == 2) & (runs < CAP).all(axis=0) & (m["ticks_run"] < 3 * CAP)
            n_fired = [int((m["leg_fired"][both, k] == cum[k, both] - 1).sum()) for k in range(2)]
            n_run = int((m["ticks_run"][both] == cum[2, both]).sum())
            say(f"  waves {waves}  chain / one launch = {med[1] / med[0]:.3f}; ticks of the slowest stream: one launch {int(m['ticks_run'].max())}, chain {' + '.join(str(int(r.max())) for r in runs)} "
                f"= {int(runs.max(axis=1).sum())}; stream-ticks {int(m['ticks_run'].sum())} against {int(runs.sum())}; records consumed per stream in the one launch: "
                f"{' '.join('%d x %d' % (int((m['legs_done'] == k).sum()), k) for k in range(3))}")
            say(f"  waves {waves}  streams that flew all three legs to their goals in both: {int(both.sum())} of {B}; leg_fired[0] = the chain's ticks_run of link 1 - 1 on {n_fired[0]} of them, "
                f"leg_fired[1] = links 1 + 2 - 1 on {n_fired[1]}, ticks_run = the sum of the three links on {n_run}; first leg ends behind ticks "
                f"{int(m['leg_fired'][both, 0].min()) if both.any() else -1}..{int(m['leg_fired'][both, 0].max()) if both.any() else -1}; the arrays of those streams at the end: "
                f"{'EQUAL bit for bit' if all(np.array_equal(fin[0][a][both], fin[1][a][both], equal_nan=True) for a in ARRAYS) else 'DIFFERENT'}")
            if part == 0 and waves == 1:
                keep = both
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sb.close(); solver.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
