"""Diagnostic (GPU): what the log of a rollout costs.  The workload of bench_stream.py's held mode (BASELINE configs[4]: 256 streams, N = 10, S = 4, 130
ticks = tick 0 solved out + 129 ticks at five iterations a tick, one wave per stream), HIP events around the loop, the variants alternating inside one
process, all on this tree's library:
  A  rollout()
  B  rollout(audit=True)
  C  rollout(want_log=True, log_stages=1, track=True)
  D  rollout(want_log=True, log_stages=10)
  E  the loop of tick_graph() + log(): what the log rows cost without the rollout -- every tick lasts as long as its slowest stream
and, untimed, the final arrays of A..E compared bit for bit, the rows of D against those the loop E collects, the record of C summed up.
profiles/stream_rollout_log.txt quotes the output.
Usage: python tests/gpu_stream_rollout_log.py [--reps 11] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")


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
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--ticks", type=int, default=130)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    import torch
    from boundmpc_amd import build, stream as bstream, workload
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    mpcs, recs = workload.make_streams(args.batch, seed=3)
    B, ticks, N = args.batch, args.ticks, 10
    tick_kw = dict(max_iter=5, warm_dual=True, accept_capped=True)
    variants = [("A rollout()", make(mpcs, recs), dict()),
                ("B rollout(audit=True)", make(mpcs, recs), dict(audit=True)),
                ("C rollout(want_log=True, log_stages=1, track=True)", make(mpcs, recs), dict(want_log=True, log_stages=1, track=True)),
                ("D rollout(want_log=True, log_stages=10)", make(mpcs, recs), dict(want_log=True, log_stages=N)),
                ("E loop of tick_graph() + log()", make(mpcs, recs), None)]
    init = [{a: getattr(sb, a).clone() for a in ARRAYS} for _, (_, sb), _ in variants]
    for i in init:
        for a in ("p", "x0", "x", "g"):
            i[a].zero_()
    ms, final, outs = [[] for _ in variants], [None] * len(variants), [None] * len(variants)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    loop_rows = torch.empty((ticks - 1, B, bstream.log_len(N)), dtype=torch.float64, device=variants[0][1][1].path.device)
    with torch.cuda.stream(torch.cuda.Stream()):
        for rep in range(args.reps + 2):      # rep 0: warm-up (code objects loaded, workspace allocated, the tick graph captured); the last: untimed, rows collected
            collect = rep == args.reps + 1
            for v, (name, (solver, sb), kw) in enumerate(variants):
                for a in ARRAYS:
                    getattr(sb, a).copy_(init[v][a])
                torch.cuda.synchronize()
                ev[0].record()
                sb.tick(max_iter=100, warm_dual=True, simulate=True)
                if kw is not None:
                    out = sb.rollout(ticks - 1, **kw, **tick_kw)
                else:
                    out = {}
                    for t in range(ticks - 1):
                        sb.tick_graph(simulate=True, **tick_kw)
                        row = sb.log()
                        if collect:
                            loop_rows[t].copy_(row)
                ev[1].record(); ev[1].synchronize()
                if rep and not collect:
                    ms[v].append(ev[0].elapsed_time(ev[1]))
                final[v], outs[v] = {a: getattr(sb, a).cpu().numpy().copy() for a in ARRAYS}, {k: t_.cpu().numpy() for k, t_ in out.items()}
    say(f"cost of the rollout log: held mode, B = {B} streams, N = 10, S = 4, tick 0 + {ticks - 1} ticks, one wave per stream, {args.reps} alternating repetitions, "
        f"source hash {build.source_hash()}; HIP events around the loop")
    med = []
    for v, (name, _, _) in enumerate(variants):
        x = np.array(ms[v]); med.append(float(np.median(x)))
        say(f"{name:52s} median {np.median(x):8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f}, spread {x.max() - x.min():5.2f})   runs: {' '.join('%.2f' % y for y in x)}")
    for v, (name, _, _) in enumerate(variants[1:], 1):
        say(f"{name[:1]} / A = {med[v] / med[0]:.4f}  ({med[v] - med[0]:+.2f} ms)")
    say(f"E / D = {med[4] / med[3]:.3f}: the rows of every stage of every tick, loop against rollout")
    run = outs[0]["ticks_run"]
    say(f"stream-ticks run {int(run.sum()) + B}; ticks_run equal in A..D: " + str(all(np.array_equal(o["ticks_run"], run) for o in outs[:4])))
    ok = True
    for v in range(1, len(variants)):
        same = all(np.array_equal(final[v][a], final[0][a], equal_nan=True) for a in ARRAYS) and (v == 4 or np.array_equal(outs[v]["hist"], outs[0]["hist"], equal_nan=True))
        say(f"final arrays{'' if v == 4 else ' and hist'}, {variants[v][0][:1]} against A: {'EQUAL bit for bit' if same else 'DIFFERENT'}")
        ok = ok and (same or v == 4)      # (the loop skips lost streams instead of stopping them: the same arrays as long as the contract holds; reported, not required)
    # the rows of D against the loop's, for the ticks D ran (the loop writes rows of skipped streams, the rollout NaN)
    rows_d, rows_e = outs[3]["log_hist"], loop_rows.cpu().numpy()
    ran = np.arange(ticks - 1)[:, None] < run[None, :]
    same_nan = np.array_equal(np.isnan(rows_d[ran]), np.isnan(rows_e[ran]))
    dev = float(np.nanmax(np.abs(rows_d[ran] - rows_e[ran])))
    say(f"log rows of D against the loop's, {int(ran.sum())} rows: NaN pattern equal {same_nan}, largest deviation {dev:.3e}, bit-equal {np.array_equal(rows_d[ran], rows_e[ran], equal_nan=True)}; "
        f"rows behind a stop all NaN: {bool(np.isnan(rows_d[~ran]).all())}")
    ok = ok and same_nan and dev <= 1e-11 and bool(np.isnan(rows_d[~ran]).all())
    say("rows of C are the prefix and trailer of D's: " + str(np.array_equal(outs[2]["log_hist"], np.concatenate([rows_d[..., :88], rows_d[..., -4:]], axis=-1), equal_nan=True)))
    trk, TR = outs[2]["track"], bstream.TRACK
    want = bstream.track_of_rows(outs[2]["log_hist"], outs[2]["hist"])
    ints = [0, 2, 5, 8, 10, 11]
    t_ok = np.array_equal(trk[:, ints], want[:, ints]) and np.allclose(np.delete(trk, ints, axis=1), np.delete(want, ints, axis=1), rtol=1e-12, atol=0.0, equal_nan=True)
    n = trk[:, TR["SAMPLES"]].sum()
    say(f"tracking record of C: {int(n)} samples, {int(trk[:, TR['REPLAYED']].sum())} replays; largest ||e_p_orth|| {np.nanmax(trk[:, TR['MAX_EP_ORTH']]):.3e} m, ||e_p_par|| "
        f"{np.nanmax(trk[:, TR['MAX_EP_PAR']]):.3e} m, ||e_r|| {np.nanmax(trk[:, TR['MAX_ER']]):.3e} rad; rms over all samples {np.sqrt(trk[:, TR['SUMSQ_EP_ORTH']].sum() / n):.3e} m, "
        f"{np.sqrt(trk[:, TR['SUMSQ_EP_PAR']].sum() / n):.3e} m, {np.sqrt(trk[:, TR['SUMSQ_ER']].sum() / n):.3e} rad; equals stream.track_of_rows: {t_ok}")
    ok = ok and t_ok
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for _, (solver, sb), _ in variants:
        sb.close(); solver.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
