"""Diagnostic (GPU box): the fixed barrier level on the REFERENCE's own two experiments through the stream API (duals and rejected iterates carried, first tick
solved out, K Newton steps per tick): which level still reaches the goal (phi_max - phi <= 0.01)?  Usage: python tests/gpu_fixed_level_experiments.py"""
import os, sys, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from boundmpc_amd import BatchedOCPSolver, stream as bstream
from tests.closed_loop import reference_experiment_streams
mpcs, recs, _ = reference_experiment_streams()
def run(label, K, feas, ticks=300, **kw):
    slv = BatchedOCPSolver(10, 4, 0.1, **kw); slv.set_rt_feasibility_tol(feas)
    sb = bstream.StreamBatch(slv, mpcs); sb.set_robot(recs)
    done=[None,None]; app=[]; best=[9.0,9.0]; lv=[]
    for t in sb.closed_loop(ticks, cap=K, accept_capped=bool(K)):
        phi = sb.phi().cpu().numpy(); app.append(sb.applied().cpu().numpy().copy())
        lv.append(sb.level().cpu().numpy().copy())
        for b in range(2):
            best[b] = min(best[b], float(mpcs[b].phi_max[0] - phi[b]))
            if done[b] is None and mpcs[b].phi_max[0] - phi[b] <= 0.01: done[b]=t+1
        if all(d is not None for d in done): break
    phi = sb.phi().cpu().numpy()
    print(label, "ticks to the goal (exp1, exp2):", done, "applied fraction", np.mean(app,axis=0).round(3).tolist(), "phi", phi.round(3).tolist(), "of", [float(m.phi_max[0]) for m in mpcs], "valid", sb.valid().double().tolist(), "closest approach", [round(v, 4) for v in best], "level in the dual state at ticks 1, 50, 100, last", [np.round(lv[i], 4).tolist() for i in (1, min(50, len(lv) - 1), min(100, len(lv) - 1), len(lv) - 1)], flush=True)
    sb.close(); slv.close()
run("converged", 0, 1e-4)
for L in (0.1, 0.01):
    for K in (8,):
        run(f"level {L} K={K} rule 1e-2", K, 1e-2, tol=1e-3, max_iter=30, fixed_barrier=L)
run("level 0.1 K=8 rule 1e-4", 8, 1e-4, tol=1e-3, max_iter=30, fixed_barrier=0.1)
for c in (0.02, 0.05, 0.1):      # the level that sets itself: clamp(c (phi_max - phi), 0.01, 0.1) per stream, held inside the tick
    for K in (8,):
        run(f"level auto c={c} K={K} rule 1e-2", K, 1e-2, tol=1e-3, max_iter=30, fixed_barrier="auto", level_c=c)
