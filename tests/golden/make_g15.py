"""Fixture g15_scipy_margin.npz: INDEPENDENT solutions of two benchmark problems under bound_margin = 0.05.

scipy's SLSQP (oracle/solve_scipy_batch.solve: dense SQP on the reference's own NLP form, nothing in common with the interior-point /
Riccati solver) with lbx / ubx of the joint positions and velocities moved inwards by the margin (oracle/solve_scipy.tighten), from the cold
start the product gets.  The problems are the first two of workload.make_batch(16, seed=0) whose oracle solution at the margin has a
margin-less KKT certificate E >= 1e-3 (tests/test_kkt_certificate.checker): there the margin moves the minimiser, so a solver that forgets it lands
somewhere else.  Our own oracle's output, like g8.

  python tests/golden/make_g15.py        (minutes)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from boundmpc_amd import workload  # noqa: E402
from oracle import c_oracle, nlp  # noqa: E402
from oracle.solve_scipy_batch import solve  # noqa: E402
from tests.test_kkt_certificate import checker  # noqa: E402

M, N, S, H = 0.05, 10, 4, 0.1


def _job(job):
    p, x0 = job
    res = solve(p, x0, N=N, maxiter=1000, bound_margin=M)
    f, g = nlp.nlp_eval(res.x, p, N, S, H)
    g2 = g.reshape(N, 43)
    print(f"{res.message} nit {res.nit} f {f:.10g} eq {np.abs(g2[:, :36]).max():.1e} ineq {g2[:, 36:].max():.1e}", flush=True)
    return res.x, f, res.nit, bool(res.success)


if __name__ == "__main__":
    import multiprocessing as mp
    P, X, _ = workload.make_batch(16, seed=0, workers=1)
    r = c_oracle.solve(P, X, N, S, H, c_oracle.default_opts(tol=1e-8, bound_margin=M), nthreads=4)
    E0 = np.array([checker(P[b], r["x"][b], r["lam_g"][b], r["lam_x"][b], N, S)[0]["E"] for b in range(16)])
    idx = np.flatnonzero((r["status"] == 0) & (E0 >= 1e-3))[:2]
    assert len(idx) == 2, E0
    with mp.get_context("fork").Pool(2) as pool:
        out = pool.map(_job, [(P[b], X[b]) for b in idx], chunksize=1)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g15_scipy_margin.npz"), idx=idx, p=P[idx], x0=X[idx], x=np.array([o[0] for o in out]),
                        f=np.array([o[1] for o in out]), nit=np.array([o[2] for o in out]), success=np.array([o[3] for o in out]), m=M)
    print("problems", idx, "margin-less E of the oracle's margin solutions", E0[idx])
