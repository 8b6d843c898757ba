"""Diagnostic (GPU box), verdict round 5 item 6c: "a polish from the level's iterate toward tolerance for the plan that is applied, while the level's iterate
stays the carrier of the warm start".  256 streams x 130 ticks with the three-kernel tick (pack, solves, post; not fused: the tick times are upper
bounds): per tick KL Newton steps on the held level (the carrier: iterate + dual state), then P more steps FROM the carrier with the barrier walking down
(a second handle, a copy of the dual state); the polished plan is judged and applied, the carrier (variant "carrier") or the accepted plan (variant
"plan") is what the next tick shifts.  Reported against the loops solved to 1e-8: plans kept, streams within 1e-2 rad RMS, tube excess.
Usage: python tests/gpu_polish_experiment.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload  # noqa: E402

B, T, N = 256, 131, 10
mpcs, recs = workload.make_streams(B, seed=3)
torch.cuda.set_stream(torch.cuda.Stream())


def loop(mode, KL=5, P=0, carrier=False, level="auto", pol_tol=1e-3):
    conv = mode == "converged"
    slv = BatchedOCPSolver(10, 4, 0.1, max_iter=100, stall_window=16) if conv else BatchedOCPSolver(10, 4, 0.1, tol=1e-3, max_iter=30, fixed_barrier=level, bound_margin=2e-3)
    pol = BatchedOCPSolver(10, 4, 0.1, tol=pol_tol, max_iter=30, mu_init=0.1, mu_warm=1e-5, bound_margin=2e-3) if P else None
    for s in (slv, pol):
        if s is not None:
            s.set_rt_feasibility_tol(1e-2); s.set_rt_position_row_cap(1e-5); s.set_start_rollout(False)
    sb = bstream.StreamBatch(slv, mpcs); sb.set_robot(recs)
    Q, ms, tube = [], [], []
    outp = {}

    def polished_tick():      # pack / solve on the level / polish / post
        if carrier:
            bstream.set_continue_rejected(sb.state, N)      # always continue from sb.x (the carrier)
        sb.pack(True, None, continue_rejected=True)
        out = dict(x=sb.x, g=sb.g, iters=sb.iters, status=sb.status, kkt=sb.kkt)
        slv.solve_batch(sb.p, sb.x0, out=out, want=("g", "iters", "status", "kkt"), state=sb.dual, max_iter=KL)      # the carrier: sb.x, sb.dual
        if P:
            stp = sb.dual.clone()
            o = pol.solve_batch(sb.p, sb.x, out=outp, want=("g", "iters", "status", "kkt"), state=stp, max_iter=P)
            xc = sb.x.clone()
            sb.x.copy_(o["x"]); sb.g.copy_(o["g"]); sb.status.copy_(o["status"])
            sb.post(True, None, True)
            if carrier:
                sb.x.copy_(xc)
        else:
            sb.post(True, None, True)
    # (the converged loops: the three-kernel tick to the handle's tolerance on every tick)
    for t in sb.closed_loop(T, graph=False, fused=False, timed=not conv, tick=None if conv else polished_tick):
        if sb.tick_ms is not None:
            ms.append(sb.tick_ms)
        Q.append(sb.robot[:, :7].cpu().numpy().copy())
        if t > 0:
            tube.append(sb.tick_tube_figures()[0].max())
    alive = float(sb.valid().double().mean()); phi = float(sb.phi().mean())
    sb.close(); slv.close()
    if pol is not None:
        pol.close()
    return np.array(Q), alive, (np.array(ms) if ms else np.zeros(1)), max(tube), phi


ref, alive, _, tb, phi = loop("converged")
print(f"converged loops: plans kept {100 * alive:.1f} %, mean phi {phi:.2f}, largest position excess {tb:.1e} m", flush=True)
for name, kw in (("level auto, 5 steps (the bench mode)", dict(KL=5)),
                 ("level 3 + polish 2, next tick from the plan", dict(KL=3, P=2)),
                 ("level 3 + polish 3, next tick from the plan", dict(KL=3, P=3)),
                 ("level 3 + polish 3, next tick from the carrier", dict(KL=3, P=3, carrier=True)),
                 ("level 4 + polish 4, next tick from the carrier", dict(KL=4, P=4, carrier=True)),
                 ("level 4 + polish 4, next tick from the plan", dict(KL=4, P=4)),
                 ("level 0.1 fixed 3 + polish 3, carrier", dict(KL=3, P=3, carrier=True, level=0.1))):
    Q, alive, ms, tb, phi = loop("rt", **kw)
    dev = np.sqrt(np.mean((Q - ref) ** 2, axis=(0, 2)))
    print(f"{name:52s}: plans kept {100 * alive:.1f} %, within 1e-2 rad RMS of the converged loops {100 * (dev <= 1e-2).mean():.1f} % (median {np.median(dev):.3f} rad), "
          f"mean phi {phi:.2f}, largest position excess {tb:.1e} m, three-kernel tick p50 {np.percentile(ms, 50):.2f} / p99 {np.percentile(ms, 99):.2f} ms", flush=True)
