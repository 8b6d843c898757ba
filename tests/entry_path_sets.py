"""Problem sets and oracle runs shared by tests/test_entry_paths.py (CPU) and tests/test_gpu_entry_paths.py (GPU): a few dozen short-horizon
problems each, chosen so that the rescue mechanisms of the solver (restoration phase, second attempt) decide the outcome.  All x0 are taken as
given (start_rollout = 0), so the main phase does jam.

  A   workload.make_batch(64, seed=60, N=10), x0 = zeros
  B   fixture G12 n5s2 (N = 5, S = 2, 12 problems) + default_rng(3).normal * 0.3
  C   fixture G12 n6s5 (N = 6, S = 5, 10 problems) + default_rng(3).normal * 0.3      (S > 4: the iterate in the workspace)
  C'  the same + default_rng(3).normal * 1.0
  D   fixture g13b (38 first failing ticks of closed loops, N = 10)"""
import functools
import os

import numpy as np

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# status counts [0, 1, 2, 3] of the CPU oracle, (set, restoration mode) -> (second attempt off, cap 100); pinned by tests/test_entry_paths.py
ORACLE_COUNTS = {
    ("A", 0): ([12, 0, 52, 0], [64, 0, 0, 0]), ("A", 1): ([59, 0, 5, 0], [64, 0, 0, 0]),
    ("B", 0): ([0, 0, 11, 1], [11, 0, 0, 1]), ("B", 1): ([12, 0, 0, 0], [12, 0, 0, 0]), ("B", 2): ([1, 0, 11, 0], [12, 0, 0, 0]),
    ("C", 0): ([0, 0, 10, 0], [10, 0, 0, 0]), ("C", 1): ([10, 0, 0, 0], [10, 0, 0, 0]), ("C", 2): ([0, 0, 10, 0], [10, 0, 0, 0]),
    ("C'", 0): ([0, 0, 9, 1], [9, 0, 0, 1]), ("C'", 1): ([10, 0, 0, 0], [10, 0, 0, 0]), ("C'", 2): ([1, 0, 9, 0], [10, 0, 0, 0]),
    ("D", 0): ([0, 0, 37, 1], [0, 0, 37, 1]), ("D", 1): ([8, 0, 30, 0], [8, 0, 30, 0]),
}
# the rows on which the second attempt changes nothing (every problem converges in the first attempt with the restoration phase): there the cap must
# change nothing on the GPU either; every other row tells a present second attempt from a missing one
CAP_CHANGES_NOTHING = {("B", 1), ("C", 1), ("C'", 1)}


@functools.lru_cache(maxsize=None)
def problem_set(name):
    """-> (P, X0, N, S, dt); read-only arrays"""
    from boundmpc_amd import workload
    if name == "A":
        P, X, _ = workload.make_batch(64, seed=60, N=10)
        out = (P, np.zeros_like(X), 10, 4, 0.1)
    elif name in ("B", "C", "C'"):
        key, N, S, nz = {"B": ("n5s2", 5, 2, 0.3), "C": ("n6s5", 6, 5, 0.3), "C'": ("n6s5", 6, 5, 1.0)}[name]
        d = np.load(os.path.join(G, "g12_pack_other_sizes.npz"))
        P = np.where(np.isfinite(d[key + "_p"]), d[key + "_p"], 0.0)
        out = (P, d[key + "_x0"] + np.random.default_rng(3).normal(size=d[key + "_x0"].shape) * nz, N, S, float(d[key + "_dt"]))
    elif name == "D":
        d = np.load(os.path.join(G, "g13b_first_failures_256_streams.npz"))
        out = (np.array(d["p"]), np.array(d["x0"]), 10, 4, 0.1)
    else:
        raise KeyError(name)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(name, mode, cap):
    """The CPU oracle on a set: restoration mode, second-attempt cap, x0 as given, every other option at its default.  Computed once per process."""
    from oracle import c_oracle
    P, X, N, S, dt = problem_set(name)
    r = c_oracle.solve(P, X, N, S, dt, opts=c_oracle.default_opts(restoration=mode, start_rollout=0, retry_cap=cap), nthreads=8)
    for a in r.values():
        a.setflags(write=False)
    return r


def counts(status):
    return np.bincount(status, minlength=4).tolist()


def rms_q(x, ref, N):
    """per-row RMS of the joint angles over the horizon"""
    d = (x - ref).reshape(-1, N, 44)[:, :, 8:15]
    return np.sqrt((d ** 2).mean(axis=(1, 2)))
