"""Diagnostic (GPU box): the KKT certificate (bmpc_kkt_batch) measured -- kernel time against one solve launch on the same handle, and the
certificate of the GPU solve's own outputs on configs[1].  Prints the GPU part of profiles/kkt_certificate.txt.
Usage: python tests/gpu_kkt_certificate.py"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundmpc_amd import BatchedOCPSolver, workload
t_ = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def gpu_ms(fn, reps=5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize(); out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


print("certificate kernel vs one solve launch on the same handle (median of 5 / 3, HIP events around the call):")
for N, B, tight, seed in ((10, 1024, False, 0), (10, 8192, False, 1), (30, 8192, True, 2)):
    P, X, _ = workload.make_batch(B, seed=seed, N=N, tight=tight)
    s = BatchedOCPSolver(N, 4, 0.1)
    p, x0 = t_(P), t_(X)
    o = s.solve_batch(p, x0); torch.cuda.synchronize()
    xs, lg, lx = o["x"].clone(), o["lam_g"].clone(), o["lam_x"].clone()
    c, cw = {}, {}
    tc = gpu_ms(lambda: s.certify(p, xs, lg, lx, out=c))
    tw = gpu_ms(lambda: s.certify(p, xs, lg, lx, want=("g", "lam_g", "rj"), out=cw))
    ts = gpu_ms(lambda: s.solve_batch(p, x0, out=o), reps=3)
    print(f"  N={N} B={B}: certificate {tc:.3f} ms (with g, lam_g, rj: {tw:.3f} ms), solve {ts:.2f} ms ({100 * tc / ts:.2f} %)")
    ok = o["status"].cpu().numpy() == 0
    E, k = c["E"].cpu().numpy()[ok], o["kkt"].cpu().numpy()[ok]
    print(f"    the solve's own outputs, {int(ok.sum())} converged of {B}: E max {E.max():.3e} median {np.median(E):.3e}; E / kkt max {(E / k).max():.2f} median {np.median(E / k):.2f}; "
          f"lam_eq_gap max {c['lam_eq_gap'].cpu().numpy()[ok].max():.2e}; lam_ineq_gap max {c['lam_ineq_gap'].cpu().numpy()[ok].max():.2e}")
    s.close()
