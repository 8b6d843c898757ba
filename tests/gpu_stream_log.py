#!/usr/bin/env python3
"""Diagnostic (GPU; not a test, not part of bench.py): what the stream log costs.  256 closed-loop streams of BASELINE configs[4] (N = 10, S = 4,
the generator of bench_stream.py), brought a few ticks into their paths; then HIP events around (a) one fused tick of these streams (the
converged tick of bench_stream.py's default mode, replayed from its graph) and (b) one bmpc_stream_log launch behind it, alternating, 7 runs
each; the medians and their ratio go to the output file.
Usage: python tests/gpu_stream_log.py [--out profiles/stream_log.txt] [--batch 256] [--lead 20]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_log.txt"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lead", type=int, default=20, help="closed-loop ticks ahead of the timed ones")
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    from boundmpc_amd import BatchedOCPSolver, build, stream as bstream, workload
    B = args.batch
    mpcs, recs = workload.make_streams(B, seed=3)
    solver = BatchedOCPSolver(10, 4, 0.1, tol=1e-8, mu_warm=1e-2, max_iter=100, stall_window=16)      # the handle of bench_stream.py's converged mode
    solver.set_restoration(cap=24)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    torch.cuda.synchronize()
    tick_ms, log_ms = [], []
    with torch.cuda.stream(torch.cuda.Stream()):
        for _ in sb.closed_loop(args.lead, cap=0, warm=False):
            pass
        sb.log(); torch.cuda.synchronize()      # (the buffer and the kernel's code object are in place before the timed launches)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        for _ in range(args.runs):
            ev[0].record()
            sb.tick_graph(max_iter=0, warm_dual=False, simulate=True)
            ev[1].record()
            sb.log()
            ev[2].record(); ev[2].synchronize()
            tick_ms.append(ev[0].elapsed_time(ev[1])); log_ms.append(ev[1].elapsed_time(ev[2]))
        rows = sb.log(); torch.cuda.synchronize()
        n_valid = rows[:, -4].cpu().numpy()
    tick, log = float(np.median(tick_ms)), float(np.median(log_ms))
    text = ("stream log against the fused tick, HIP events, B = %d streams, N = 10, S = 4, source hash %s\n"
            "(%d closed-loop ticks ahead; then tick and log alternating, median of %d)\n"
            "fused tick (converged mode, graph replay)   %.4f ms   (runs: %s)\n"
            "bmpc_stream_log                             %.4f ms   (runs: %s)\n"
            "log / tick                                  %.4f\n"
            "streams with a plan in the last log: %d of %d\n"
            % (B, build.source_hash(), args.lead, args.runs, tick, " ".join("%.4f" % v for v in tick_ms), log, " ".join("%.4f" % v for v in log_ms),
               log / tick, int((n_valid > 0).sum()), B))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    sb.close(); solver.close()


if __name__ == "__main__":
    main()
