"""Diagnostic (GPU): what the audit of a rollout costs.  The workload of bench_stream.py's held mode (BASELINE configs[4]: 256 streams, N = 10, S = 4, 130
ticks = tick 0 solved out + a rollout of 129 ticks at five iterations a tick, one wave per stream), HIP events around the loop, the variants
alternating inside one process:
  A  bmpc_stream_rollout_events without an event, library of the PARENT commit (--parent-lib: an A/B build of it; left out without)
  B  the same entry, this tree's library
  C  bmpc_stream_rollout_audit with tube_hist and audit, this tree's library
and the final arrays of B and C compared bit for bit, the audit summed up.  Run it twice (two processes); profiles/stream_audit.txt quotes the output.
Usage: python tests/gpu_stream_audit.py [--parent-lib PATH] [--reps 11] [--out FILE]"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ARRAYS = ("state", "robot", "p", "x0", "dual", "x", "g", "iters", "status", "kkt", "traj")


def _bind(path):
    """a second library beside the tree's, with the signatures it has (an older revision lacks entry points)"""
    from boundmpc_amd import _lib
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    return lib


def make(mpcs, recs, lib=None):
    from boundmpc_amd import BatchedOCPSolver, _lib, stream as bstream
    mine = _lib.load()
    if lib is not None:
        _lib._lib = lib          # the handle is created by, and keeps, the library it is given
    try:
        solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-3, max_iter=30, fixed_barrier="auto", bound_margin=2e-3)
    finally:
        _lib._lib = mine
    solver.set_rt_feasibility_tol(1e-2); solver.set_rt_position_row_cap(1e-5)
    solver.set_team_waves(1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    return solver, sb


def events_entry_without_events(sb, ticks, max_iter, warm_dual, accept_capped):
    """bmpc_stream_rollout_events with every event pointer NULL on the buffers of `sb` (StreamBatch.rollout calls the plain entry then)"""
    import torch
    from boundmpc_amd import _lib, stream as bstream
    from boundmpc_amd.solver import _ptr
    dev = sb.path.device
    out = {"hist": torch.empty((ticks, sb.B, bstream.ROLL["LEN"]), dtype=torch.float64, device=dev), "ticks_run": torch.zeros((sb.B,), dtype=torch.int32, device=dev)}
    args = sb._tick_args(max_iter, warm_dual, True, accept_capped)
    _lib.check(sb.solver._lib.bmpc_stream_rollout_events(sb.solver._h, args[0], ticks, *args[1:], 0.0, _ptr(out["hist"]), None, _ptr(out["ticks_run"]), None, None, None, 3, None,
                                                         sb._stream(None)), "bmpc_stream_rollout_events")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
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
    B, ticks = args.batch, args.ticks
    tick_kw = dict(max_iter=5, warm_dual=True, accept_capped=True)
    variants = []
    if args.parent_lib:
        parent = _bind(args.parent_lib)
        variants.append((f"A parent commit ({parent.bmpc_build_hash().decode()}), rollout_events, no event", make(mpcs, recs, parent), None))
    variants.append(("B this commit, rollout_events, no event", make(mpcs, recs), None))
    variants.append(("C this commit, rollout_audit, tube_hist + audit, no event", make(mpcs, recs), dict(audit=True, want_tube=True)))
    init = [{a: getattr(sb, a).clone() for a in ARRAYS} for _, (_, sb), _ in variants]
    for i in init:
        for a in ("p", "x0", "x", "g"):
            i[a].zero_()
    ms, final, outs = [[] for _ in variants], [None] * len(variants), [None] * len(variants)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    with torch.cuda.stream(torch.cuda.Stream()):
        for rep in range(args.reps + 1):      # rep 0: warm-up (code objects loaded, workspace allocated)
            for v, (name, (solver, sb), kw) in enumerate(variants):
                for a in ARRAYS:
                    getattr(sb, a).copy_(init[v][a])
                torch.cuda.synchronize()
                ev[0].record()
                sb.tick(max_iter=100, warm_dual=True, simulate=True)
                out = events_entry_without_events(sb, ticks - 1, **tick_kw) if kw is None else sb.rollout(ticks - 1, **kw, **tick_kw)
                ev[1].record(); ev[1].synchronize()
                if rep:
                    ms[v].append(ev[0].elapsed_time(ev[1]))
                final[v], outs[v] = {a: getattr(sb, a).cpu().numpy().copy() for a in ARRAYS}, {k: t.cpu().numpy() for k, t in out.items()}
    say(f"cost of the rollout audit: held mode, B = {B} streams, N = 10, S = 4, tick 0 + rollout of {ticks - 1} ticks, one wave per stream, {args.reps} alternating "
        f"repetitions, source hash {build.source_hash()}; HIP events around the loop")
    med = []
    for v, (name, _, _) in enumerate(variants):
        x = np.array(ms[v]); med.append(float(np.median(x)))
        say(f"{name:58s} median {np.median(x):8.2f} ms  (min {x.min():8.2f}, max {x.max():8.2f}, spread {x.max() - x.min():5.2f})   runs: {' '.join('%.2f' % y for y in x)}")
    base = med[0]
    for v, (name, _, _) in enumerate(variants[1:], 1):
        say(f"{name[:1]} / {variants[0][0][:1]} = {med[v] / base:.4f}  ({med[v] - base:+.2f} ms)")
    run = outs[-1]["ticks_run"]
    say(f"stream-ticks run {int(run.sum()) + B} in every variant: " + str(all(np.array_equal(o["ticks_run"], run) for o in outs)))
    for v in range(len(variants) - 1):
        same = all(np.array_equal(final[v][a], final[-1][a], equal_nan=True) for a in ARRAYS) and np.array_equal(outs[v]["hist"], outs[-1]["hist"], equal_nan=True)
        say(f"final arrays and hist, {variants[v][0][:1]} against C: {'EQUAL bit for bit' if same else 'DIFFERENT'}")
    tube, audit = outs[-1]["tube_hist"], outs[-1]["audit"]
    A = bstream.AUDIT
    samples = int(audit[:, A["SAMPLES"]].sum())
    say(f"audit (tolerance 1e-6): {samples} samples; outside the position tube {int(audit[:, A['N_POS']].sum())}, the orientation tube {int(audit[:, A['N_ROT']].sum())}, "
        f"a joint limit {int(audit[:, A['N_JOINT']].sum())}; largest position excess {np.nanmax(audit[:, A['MAX_POS']]):.3e} m, orientation {np.nanmax(audit[:, A['MAX_ROT']]):.3e} rad; "
        f"streams ever outside a tube {int((audit[:, A['FIRST_OUT']] >= 0).sum())} of {B}")
    ok = bool((np.isnan(tube[:, :, bstream.TUBE['SEG']]).sum(axis=0) == ticks - 1 - run).all()) and samples == int(run.sum())
    say("NaN rows and SAMPLES agree with ticks_run: " + str(ok))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for _, (solver, sb), _ in variants:
        sb.close(); solver.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
