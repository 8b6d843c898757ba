"""Random interior points (p, x, t, nu, mu) for the tests of ONE Newton direction (tests/test_emu.py, tests/test_newton_step.py): a seeded
problem of the synthetic generator for any (N, S), its cold start moved off the dynamics by Gaussian noise of 0.02 on every variable, the path
parameter moved inside its bound, slacks t = max(-h, 1e-2) and multipliers nu = (mu / t) 10^U(-2, 2) -- the barrier ratios nu / t then span more
than six decades (jerk rows with t = 35 beside rows at the slack floor), which sigma_spread() reports and the tests assert."""
import numpy as np

MU = 0.1
H_ = 0.1


def interior_point(N, S, seed):
    from boundmpc_amd import workload
    from oracle import nlp
    P, X, _ = workload.make_batch(1, seed=seed, N=N, S=S, workers=1)
    p, rng = P[0], np.random.default_rng(1000 + seed)
    x = X[0] + rng.normal(size=44 * N) * 0.02
    phi = x.reshape(N, 44)[:, nlp.IPHI]
    phi[:] = np.abs(phi) + 0.05      # inside phi >= 0, and far from the first segment switch of these paths (1.86) and from phi_max
    hin = nlp.internal_ineq(x, p, N, S)
    t = np.maximum(-hin, 1e-2)
    nu = MU / t * 10.0 ** rng.uniform(-2, 2, t.shape)
    return p, x, t, nu, MU


def sigma_spread(t, nu):
    """decades between the smallest and the largest barrier ratio nu / t"""
    sg = nu / t
    return float(np.log10(sg.max() / sg.min()))


def first_point_that_factorises(N, S, delta, exact=1, seed0=0, tries=32):
    """The first seed >= seed0 at whose interior point the ORACLE's factorisation succeeds with this delta (at delta = 0 an indefinite stage
    block is common this far from a solution; the solver would regularise) -> (seed, point).  The choice looks at the oracle's return code only."""
    from oracle import c_oracle
    for seed in range(seed0, seed0 + tries):
        pt = interior_point(N, S, seed)
        if c_oracle.debug_qp(*pt, N, S, H_, exact, delta)["rc"] == 0:
            return seed, pt
    raise AssertionError(f"no point among seeds {seed0}..{seed0 + tries - 1} factorises at delta {delta} (N {N}, S {S})")
