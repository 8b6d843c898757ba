"""Diagnostic (CPU): "a converged solve certifies" -- the C oracle's tol-1e-8 solutions of the fixture problems of tests/test_kkt_certificate.py
(g6 tick 0 and the G7 ticks of both experiments, a 64-problem sample of BASELINE configs[1]) certified by that file's numpy checker.  Prints the
`key = value` lines of the CPU part of profiles/kkt_certificate.txt (test_measured_a_converged_solve_certifies recomputes them; the GPU suite reads
max_E_over_tol).  Usage: python tests/kkt_certificate_profile.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import c_oracle      # noqa: E402
from tests.test_kkt_certificate import certify_oracle_solutions, fixture_problems, measured_lines      # noqa: E402

P, X = fixture_problems()
r = c_oracle.solve(P, X, 10, 4, 0.1, c_oracle.default_opts(tol=1e-8), nthreads=8)
ok, E, lines = measured_lines(P, X, r)
print("\n".join(lines))
_, at_sol, at_x0 = certify_oracle_solutions(P, X, r)
for k in ("dual", "prim_eq", "prim_ineq", "compl", "lam_eq_gap", "lam_ineq_gap"):
    v = np.array([c[0][k] for c in at_sol])
    print(f"at the solutions: {k} median {np.median(v):.3e} max {v.max():.3e}")
E0 = np.array([c[0]["E"] for c in at_x0])
print(f"E at the starts (no multipliers): min {E0.min():.3e} median {np.median(E0):.3e}; largest E(solution) / E(start) {(E / E0).max():.3e}")
