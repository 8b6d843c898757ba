"""Diagnostic (GPU): what a table of controller settings per stream costs inside a rollout and what a sweep in one launch saves.  The workload of
bench_stream.py's held mode (BASELINE configs[4]: N = 10, S = 4, tick 0 solved out, then five iterations a tick under the real-time rule), on one wave
per stream and on teams of four, the variants alternating inside one process, all on this tree's library, medians of 7:
  (i)   cost of the table: bmpc_stream_rollout_tuned with a table of NaN against bmpc_stream_rollout_legs on identical arguments (256 streams, legs = 1:
        a re-plan with splice behind tick 64 of every stream, tracking record on), 129 ticks, HIP events around the launch; the final arrays compared
        bit for bit.  The legs kernels are the parent's: the baseline in the same build.
  (ii)  what a sweep saves: 16 settings x 16 streams as ONE tuned launch of 256 streams against the same work as 16 launches of 16 streams on 16 handles
        set up from tune_used, enqueued back to back on one stream; wall time box to box (synchronised at both ends); every stream compared bit for bit.
  (iii) a demonstration, reported only: that grid -- (LVL_C, LVL_LO, cap, RT_TOL) on copies of the first 16 benchmark streams, track and audit on --,
        one line per setting: plans kept, goals reached (phi_max - phi <= 0.02 at the end), largest tube excess.
profiles/stream_rollout_tune.txt quotes the output.
Usage: python tests/gpu_stream_rollout_tune.py [--reps 7] [--out FILE]"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj", "path")
GOAL = 0.02
GRID = dict(lvl_c=(0.02, 0.05), lvl_lo=(0.01, 0.03), max_iter=(3, 5), rt_tol=(1e-2, 1e-3))


def make(mpcs, recs):
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-3, max_iter=30, fixed_barrier="auto", bound_margin=2e-3)
    solver.set_rt_feasibility_tol(1e-2); solver.set_rt_position_row_cap(1e-5)
    solver.set_team_waves(1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    return solver, sb


def make_from(row, mpcs):
    """a batch on a handle of its own whose options and setters carry the resolved row"""
    from boundmpc_amd import BatchedOCPSolver, _lib, stream as bstream
    u = bstream.unpack_tune(row)
    s = BatchedOCPSolver(10, 4, 0.1, tol=u["tol"], max_iter=u["max_iter"], mu_init=u["mu_init"], slack_push=u["slack_push"], mu_warm=u["mu_warm"], stall_window=u["stall_window"],
                         bound_margin=u["bound_margin"], mu_min_fac=u["mu_min_fac"])
    _lib.check(s._lib.bmpc_set_barrier_hold(s._h, u["hold"]), "bmpc_set_barrier_hold")
    _lib.check(s._lib.bmpc_stream_set_level_rule(s._h, u["lvl_c"], u["lvl_lo"], u["lvl_hi"]), "bmpc_stream_set_level_rule")
    s.set_rt_feasibility_tol(u["rt_tol"]); s.set_rt_position_row_cap(u["rt_row_cap"])
    s.set_team_waves(1)
    return s, bstream.StreamBatch(s, mpcs)


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
    same = lambda x, y, rows=slice(None): all(np.array_equal(x[a][rows], y[a], equal_nan=True) for a in ARRAYS)
    say(f"sweeps inside a rollout: held mode, N = 10, S = 4, behind a solved-out tick 0, {n} ticks, {args.reps} alternating repetitions, source hash {build.source_hash()}")

    # ---- (i) cost of the table ----
    mpcs, recs = workload.make_streams(B, seed=3)
    solver, sb = make(mpcs, recs)
    back, at = leg_records(mpcs, recs, sb.entries), np.full(B, 64)
    sb.tick(max_iter=100, warm_dual=True, simulate=True)
    torch.cuda.synchronize()
    init = {a: getattr(sb, a).clone() for a in ARRAYS}

    def restore(batch, state):
        for a in ARRAYS:
            getattr(batch, a).copy_(state[a])
        torch.cuda.synchronize()

    def final(batch):
        torch.cuda.synchronize()
        return {a: getattr(batch, a).cpu().numpy().copy() for a in ARRAYS}
    say(f"(i) a table of NaN against the legs entry on identical arguments: B = {B} benchmark streams, legs = 1 (a re-plan with splice behind tick 64 of every stream), track=True; "
        f"HIP events around the launch")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    nan = torch.full((B, bstream.TUNE["LEN"]), float("nan"), dtype=torch.float64, device=sb.path.device)
    legs = dict(legs=back[:, None], leg_tick=at[:, None])
    for waves in (1, 4):
        variants = [("legs entry   rollout(legs=, leg_tick=)", legs), ("tuned entry  rollout(legs=, leg_tick=, tune=NaN)", dict(legs, tune=nan)), ("legs entry   again (the spread of its own runs)", legs)]
        ms, fin, outs = [[] for _ in variants], [None] * 3, [None] * 3
        for rep in range(args.reps + 1):      # rep 0: warm-up
            for v, (_, kw) in enumerate(variants):
                restore(sb, init)
                ev[0].record()
                out = sb.rollout(n, track=True, waves=waves, **kw, **tick_kw)
                ev[1].record(); ev[1].synchronize()
                if rep:
                    ms[v].append(ev[0].elapsed_time(ev[1]))
                fin[v], outs[v] = final(sb), {k: t.cpu().numpy() for k, t in out.items()}
        med = [float(np.median(m)) for m in ms]
        for v, (name, _) in enumerate(variants):
            x = np.array(ms[v])
            say(f"  waves {waves}  {name:50s} median {med[v]:8.3f} ms  (min {x.min():8.3f}, max {x.max():8.3f}, spread {x.max() - x.min():6.3f} = {(x.max() - x.min()) / med[v] * 100:.2f} %)   "
                f"runs: {' '.join('%.3f' % y for y in x)}")
        pooled = np.array(ms[0] + ms[2])
        say(f"  waves {waves}  tuned / legs = {med[1] / med[0]:.4f} ({med[1] - med[0]:+.3f} ms = {(med[1] - med[0]) / n * 1e3:+.2f} us a tick); the legs entry against itself {med[2] / med[0]:.4f}; "
            f"spread of the legs entry's {len(pooled)} runs {(pooled.max() - pooled.min()) / np.median(pooled) * 100:.2f} % of their median [{pooled.min():.3f}, {pooled.max():.3f}]; the tuned "
            f"median lies {'INSIDE' if pooled.min() <= med[1] <= pooled.max() else 'OUTSIDE'} it")
        eq = same(fin[0], fin[1]) and all(np.array_equal(outs[0][k], outs[1][k], equal_nan=True) for k in ("hist", "ticks_run", "track", "replan_info", "legs_done", "leg_fired"))
        say(f"  waves {waves}  final arrays, path tables, hist, ticks_run, track, replan_info, legs_done, leg_fired: {'EQUAL bit for bit' if eq else 'DIFFERENT'}; tune_info all 0: "
            f"{bool((outs[1]['tune_info'] == 0).all())}; stream-ticks {int(outs[1]['ticks_run'].sum())}")
    sb.close(); solver.close()

    # ---- (ii), (iii) a grid of 16 settings on copies of 16 streams ----
    names = list(GRID)
    grid = list(itertools.product(*GRID.values()))
    K, M = len(grid), B // len(grid)
    mp, rc = workload.make_streams(M, seed=3)
    mpcs, recs = [mp[i % M] for i in range(K * M)], np.concatenate([rc] * K)      # setting k: streams k M .. k M + M - 1
    table = bstream.tune_table(K * M, **{nm: np.repeat([g[j] for g in grid], M) for j, nm in enumerate(names)})
    solver, sb = make(mpcs, recs)
    sb.tick(max_iter=100, warm_dual=True, simulate=True)
    torch.cuda.synchronize()
    init = {a: getattr(sb, a).clone() for a in ARRAYS}
    tdev = torch.as_tensor(table, device=sb.path.device)
    probe = sb.rollout(1, tune=tdev, want_tune_used=True, **tick_kw)
    torch.cuda.synchronize()
    used = probe["tune_used"].cpu().numpy()
    handles = [make_from(used[k * M], mp) for k in range(K)]
    inits = [{a: init[a][k * M:(k + 1) * M].clone() for a in ARRAYS} for k in range(K)]
    say(f"(ii) {K} settings x {M} streams ({' x '.join(f'{nm} {GRID[nm]}' for nm in names)}; copies of the first {M} benchmark streams): ONE tuned launch of {K * M} streams against {K} "
        f"launches of {M} streams on {K} handles set up from tune_used, back to back on one stream; audit and track on; wall time box to box")
    for waves in (1, 4):
        wall, fin, res = [[], []], [None, None], [None, None]
        for rep in range(args.reps + 1):
            for v in range(2):
                if v == 0:
                    restore(sb, init)
                    t0 = time.perf_counter()
                    out = sb.rollout(n, tune=tdev, audit=True, track=True, waves=waves, **tick_kw)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    fin[0], res[0] = final(sb), {k: t.cpu().numpy() for k, t in out.items()}
                else:
                    for (_, hb), st in zip(handles, inits):
                        restore(hb, st)
                    t0 = time.perf_counter()
                    outs = [hb.rollout(n, audit=True, track=True, waves=waves, warm_dual=True, accept_capped=True) for _, hb in handles]
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    fin[1] = [final(hb) for _, hb in handles]
                    res[1] = [{k: t.cpu().numpy() for k, t in o.items()} for o in outs]
                if rep:
                    wall[v].append((t1 - t0) * 1e3)
        med = [float(np.median(w)) for w in wall]
        for v, name in enumerate((f"ONE launch   rollout(tune=) of {K * M} streams", f"{K} launches  rollout() of {M} streams on {K} handles")):
            x = np.array(wall[v])
            say(f"  waves {waves}  {name:52s} median {med[v]:8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f})   runs: {' '.join('%.2f' % y for y in x)}")
        eq = all(same(fin[0], fin[1][k], slice(k * M, (k + 1) * M)) and all(np.array_equal(res[0][q][:, k * M:(k + 1) * M] if q == "hist" else res[0][q][k * M:(k + 1) * M], res[1][k][q], equal_nan=True)
                                                                                for q in ("hist", "ticks_run", "audit", "track")) for k in range(K))
        say(f"  waves {waves}  {K} launches / one launch = {med[1] / med[0]:.3f}; every stream's final arrays, path table, hist, ticks_run, audit, track: {'EQUAL bit for bit' if eq else 'DIFFERENT'}; "
            f"tune_info all 0: {bool((res[0]['tune_info'] == 0).all())}")
        if waves == 1:
            SS, AU = bstream.SS, bstream.AUDIT
            say(f"(iii) the grid on one wave per stream, reported only ({M} streams a setting, {n} ticks behind tick 0; kept: the stream ran every tick; goal: phi_max - phi <= {GOAL} at the end; "
                f"tube excess: the audit's largest position excess over the setting's streams, m)")
            for k, g in enumerate(grid):
                rows = slice(k * M, (k + 1) * M)
                kept = int((res[0]["ticks_run"][rows] == n).sum())
                st = fin[0]["state"][rows]
                goals = int((st[:, SS["PHIMAX"]] - st[:, SS["PHI"]] <= GOAL).sum())
                say(f"  {'  '.join(f'{nm} {v:g}' for nm, v in zip(names, g)):58s} plans kept {kept:2d} of {M}   goals reached {goals:2d}   largest tube excess {np.nanmax(res[0]['audit'][rows, AU['MAX_POS']]):.3e}")
    for s, hb in handles:
        hb.close(); s.close()
    sb.close(); solver.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
