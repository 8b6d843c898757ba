"""Diagnostic (GPU box): the parametric sensitivity (bmpc_sens_batch) measured -- the kernel's discrepancy against the checked set of
tests/test_sensitivity.py, and its time at B = 1024 and 8192 next to one solve launch of the same batch and next to the two-solve finite
difference it replaces (alternating runs, medians).  Prints the GPU part of profiles/sensitivity.txt.
Usage: python tests/gpu_sensitivity.py"""
import os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boundmpc_amd import BatchedOCPSolver, workload
from tests.test_sensitivity import FACTOR, MU, _scale, floor_of, golden_rows
t_ = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")

rows = golden_rows()
fl, worst = floor_of(rows), 0.0
for N in (2, 3):
    rs = [r for r in rows if r["N"] == N]
    st = lambda k: np.stack([r[k] for r in rs])
    s = BatchedOCPSolver(N, 4, 0.1)
    o = s.sensitivity_host(st("p"), st("x"), st("dp"), lam_g=st("lam_g"), lam_x=st("lam_x"), mu=MU)
    worst = max([worst] + [np.abs(o["dx"][i] - r["dx"]).max() / _scale(r) for i, r in enumerate(rs)])
    s.close()
print(f"floor = {fl:.6e}\nbound = {FACTOR * fl:.6e}\ngpu_discrepancy = {worst:.6e}")


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(); fn(); ev[1].record(); torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


print("sensitivity kernel, one solve launch, and the two-solve finite difference on the same handle (alternating runs, median of 7, HIP events around the call):")
for B, seed in ((1024, 0), (8192, 1)):
    P, X, _ = workload.make_batch(B, seed=seed)
    rng = np.random.default_rng(seed)
    dP = np.zeros_like(P); dP[:, :7] = rng.normal(size=(B, 7))      # a measured joint state that arrives late
    s = BatchedOCPSolver(10, 4, 0.1)
    p, x0, dp = t_(P), t_(X), t_(dP)
    pp, pm = t_(P + 1e-4 * dP), t_(P - 1e-4 * dP)
    o = s.solve_batch(p, x0); torch.cuda.synchronize()
    xs, lg, lx = o["x"].clone(), o["lam_g"].clone(), o["lam_x"].clone()
    o2 = {}
    legs = {"sens": lambda: s.sensitivity(p, xs, dp, lam_g=lg, lam_x=lx), "sens+duals": lambda: s.sensitivity(p, xs, dp, lam_g=lg, lam_x=lx, want_duals=True),
            "solve": lambda: s.solve_batch(p, x0, out=o2), "two solves": lambda: (s.solve_batch(pp, x0, out=o2), s.solve_batch(pm, x0, out=o2))}
    for fn in legs.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(7):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    md = {k: float(np.median(v)) for k, v in ms.items()}
    it = float(o["iters"].double().mean())
    r = s.sensitivity(p, xs, dp, lam_g=lg, lam_x=lx)["rec"].cpu().numpy()
    ok = o["status"].cpu().numpy() == 0
    print(f"  B={B}: sensitivity {md['sens']:.3f} ms (with dlam_eq, dnu: {md['sens+duals']:.3f} ms), solve {md['solve']:.2f} ms ({it:.1f} iterations mean), two solves {md['two solves']:.2f} ms; "
          f"sensitivity / solve = {md['sens'] / md['solve']:.3f} (= {md['sens'] / md['solve'] * it:.2f} solver iterations), / two solves = {md['sens'] / md['two solves']:.3f}")
    print(f"    status of the {int(ok.sum())} converged problems: 0: {int((r[ok, 0] == 0).sum())}, 1: {int((r[ok, 0] == 1).sum())}, 3: {int((r[ok, 0] == 3).sum())}; max |dx| median {np.median(r[ok, 3]):.3e}")
    s.close()
