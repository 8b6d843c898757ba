"""Diagnostic (GPU box): the primal-dual warm start (bmpc_state_from_multipliers) measured -- conversion kernel time against one solve launch,
iterations from three starts on configs[1], the drop-in single-call latency on the G7 loops with and without multipliers, and the iterations per
tick of the reference's own hand-over (multipliers of tick t-1, unshifted, with the shifted x0).  Usage: python tests/gpu_dual_warm_start.py"""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundmpc_amd import BatchedOCPSolver, NlpSolverShim, workload
G = os.path.join(ROOT, "tests", "golden")
t_ = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def gpu_ms(fn, reps=5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize(); out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


print("conversion kernel vs one solve launch (median of 5, torch events around the call):")
for N, B, tight, seed in ((10, 256, False, 0), (10, 1024, False, 0), (10, 8192, False, 1), (30, 8192, True, 2)):
    P, X, _ = workload.make_batch(B, seed=seed, N=N, tight=tight)
    s = BatchedOCPSolver(N, 4, 0.1)
    p, x0 = t_(P), t_(X)
    o = s.solve_batch(p, x0); torch.cuda.synchronize()
    lg, lx, st = o["lam_g"].clone(), o["lam_x"].clone(), s.new_state(B)
    tc = gpu_ms(lambda: s.state_from_multipliers(p, x0, lg, lx, out=st))
    ts = gpu_ms(lambda: s.solve_batch(p, x0, out=o), reps=3)
    print(f"  N={N} B={B}: conversion {tc:.3f} ms, solve {ts:.2f} ms ({100 * tc / ts:.2f} %)")
    if N == 10 and B == 1024:
        ok = o["status"].cpu().numpy() == 0
        xs = o["x"].clone()
        a = s.solve_batch(p, xs, out={}); b = s.solve_batch(p, xs, out={}, lam_g0=lg, lam_x0=lx); torch.cuda.synchronize()
        for nm, r in (("cold", o), ("x* without multipliers", a), ("x* with multipliers", b)):
            it = r["iters"].cpu().numpy()[ok]
            print(f"  configs[1] start {nm}: iterations mean {it.mean():.2f} max {it.max()}")
    s.close()

d6s = {w: np.load(os.path.join(G, f"g6_pack_exp{w}_tick0.npz")) for w in (1, 2)}
for which in (1, 2):
    d = dict(np.load(os.path.join(G, f"g7_closedloop_exp{which}.npz")))
    s = BatchedOCPSolver(10, 4, 0.1); shim = NlpSolverShim(s)
    for _ in range(3):
        shim(x0=d["x0"][0], p=d["p"][0])
    lat = {False: [], True: []}; its = {False: [], True: []}
    lg, lx = 0, 0
    for t in range(len(d["p"])):      # the reference's hand-over: multipliers of the previous tick's solve, unshifted, with its shifted x0
        for duals in (False, True):
            t0 = time.perf_counter()
            sol = shim(x0=d["x0"][t], p=d["p"][t], lam_g0=lg, lam_x0=lx) if duals else shim(x0=d["x0"][t], p=d["p"][t])
            lat[duals].append((time.perf_counter() - t0) * 1e3); its[duals].append(shim.stats()["iter_count"])
            if duals:
                lg, lx = sol["lam_g"], sol["lam_x"]
    for duals in (False, True):
        l = np.array(lat[duals])
        print(f"experiment {which} drop-in call {'with' if duals else 'without'} multipliers over {len(l)} recorded ticks: p50 {np.percentile(l, 50):.2f} ms "
              f"p99 {np.percentile(l, 99):.2f} ms; iterations per tick mean {np.mean(its[duals]):.2f} max {max(its[duals])}")
    shim.close(); s.close()
