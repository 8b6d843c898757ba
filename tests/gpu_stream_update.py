#!/usr/bin/env python3
"""Diagnostic (GPU; not a test, not part of bench.py): what re-planning costs.  256 closed-loop streams of BASELINE configs[4] (N = 10, S = 4, the
generator of bench_stream.py), brought a few ticks into their paths; every stream gets a re-plan record (the other experiment's path from its
start pose).  HIP events around (a) one fused tick of these streams (converged mode, graph replay), (b) one bmpc_stream_update launch with every
flag raised, (c) one with no flag raised, 7 runs each; beside them the wall time of the host's way of doing (b): a loop of B StreamBatch.update
calls.  The medians and their ratios go to the output file.
Usage: python tests/gpu_stream_update.py [--out profiles/stream_update.txt] [--batch 256] [--lead 20]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEYS = ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min", "e_p_max", "e_r_max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_update.txt"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--lead", type=int, default=20, help="closed-loop ticks ahead of the timed launches")
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
    plans = []
    for b in range(B):
        p0fk = recs[b][bstream.RB["P"]:bstream.RB["P"] + 6]
        path = workload.experiment2_path(p0fk)
        plans.append([path[k] for k in KEYS] + [p0fk, np.zeros(6), np.zeros(6), np.zeros(6), p0fk, mpcs[b].weights])
    records = torch.tensor(np.stack([bstream.replan_record(4, sb.entries, *a) for a in plans]), device=sb.path.device)
    idle = records.clone(); idle[:, 0] = 0.0
    torch.cuda.synchronize()
    tick_ms, all_ms, none_ms = [], [], []
    with torch.cuda.stream(torch.cuda.Stream()):
        for _ in sb.closed_loop(args.lead, cap=0, warm=False):
            pass
        sb.update_device(idle); torch.cuda.synchronize()      # (the buffers and the kernel's code object are in place before the timed launches)
        state0, path0, robot0 = sb.state.clone(), sb.path.clone(), sb.robot.clone()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for _ in range(args.runs):
            sb.state.copy_(state0); sb.path.copy_(path0); sb.robot.copy_(robot0)      # every run from the same streams, not yet re-planned
            sb.replan.copy_(records); torch.cuda.synchronize()
            ev[0].record()
            sb.tick_graph(max_iter=0, warm_dual=False, simulate=True)
            ev[1].record()
            sb.update_device(sb.replan)
            ev[2].record()
            sb.update_device(sb.replan)                       # the first launch cleared every flag
            ev[3].record(); ev[3].synchronize()
            tick_ms.append(ev[0].elapsed_time(ev[1])); all_ms.append(ev[1].elapsed_time(ev[2])); none_ms.append(ev[2].elapsed_time(ev[3]))
        replanned = int((sb.state[:, bstream.ss_updated(10)] == 1.0).sum())
        # the host's way: one StreamBatch.update per stream (a device-wide synchronisation, the state row to the host, ReferencePath, table and row back)
        sb.state.copy_(state0); sb.path.copy_(path0); sb.robot.copy_(robot0); torch.cuda.synchronize()
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for b in range(B):
                sb.update(b, *plans[b])
            torch.cuda.synchronize()
            host_ms.append(1e3 * (time.perf_counter() - t0))
    tick, upd, idl, host = (float(np.median(v)) for v in (tick_ms, all_ms, none_ms, host_ms))
    fmt = lambda v: " ".join("%.4f" % x for x in v)
    text = ("stream re-planning against the fused tick, B = %d streams, N = 10, S = 4, paths of 5 via points, source hash %s\n"
            "(%d closed-loop ticks ahead; then tick, update with every flag raised, update with none, HIP events, median of %d)\n"
            "fused tick (converged mode, graph replay)        %.4f ms   (runs: %s)\n"
            "bmpc_stream_update, %3d flags raised             %.4f ms   (runs: %s)\n"
            "bmpc_stream_update, no flag raised               %.4f ms   (runs: %s)\n"
            "update / tick                                    %.4f\n"
            "loop of %d StreamBatch.update calls (host, wall) %.1f ms   (runs: %s)\n"
            "host loop / tick                                 %.1f\n"
            "host loop / device launch                        %.0f\n"
            "streams re-planned by the last flagged launch: %d of %d\n"
            % (B, build.source_hash(), args.lead, args.runs, tick, fmt(tick_ms), B, upd, fmt(all_ms), idl, fmt(none_ms), upd / tick, B, host,
               " ".join("%.1f" % x for x in host_ms), host / tick, host / upd, replanned, B))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    sb.close(); solver.close()


if __name__ == "__main__":
    main()
