"""ONE Newton direction at interior points far from a solution, without a GPU: the C oracle's (bmpc_oracle_debug_qp) and the kernel text's
(tests/emu bmpc_emu_newton, every wave program) against an independent dense reference (tests/newton_reference.py: numpy.linalg on derivatives
taken through oracle/nlp.py), and against each other.

THE POINTS (tests/newton_points.py): a seeded generator problem per (N, S), its cold start with Gaussian noise 0.02 on every variable, slacks
t = max(-h, 1e-2), multipliers (mu / t) 10^U(-2, 2): nu / t spans more than six decades (asserted).  delta = 10: the point of seed 0.
delta = 0: the first seed (from 0 upwards) at which the ORACLE's factorisation succeeds without regularisation
(newton_points.first_point_that_factorises; this far from a solution an indefinite stage block is common, and the solver regularises) -- the
choice reads the oracle's return code and nothing else.

TOLERANCE (measured, not picked; none comes from what the code under test gives).  The reference is computed twice, with the step 1e-3 and
2e-3 of its five-point central difference; the largest discrepancy of the two relative to max |dZ| is the FLOOR of that point: the truncation
and rounding noise of the differenced second derivatives, amplified by the system.  Oracle and kernel text must agree with the reference within
FACTOR = 100 x floor -- the factor and the reasoning of tests/test_sensitivity.py: summation order, and the factorisation of a matrix whose
sigma spans many decades.  The floor is recomputed on every run; tests/newton_step_profile.py writes it with the observed discrepancies to
profiles/newton_step.txt.

KERNEL TEXT AGAINST ORACLE: dZ, the gains KT and the feed-forward KF with the bound of tests/test_emu.py's direction test, 1e-12, relative to
max(1, largest entry of the oracle's array): at delta = 10 the entries are below 1 and the bound is that test's; the unregularised systems have
gains of 1e2 .. 7e3, where an absolute 1e-12 would ask for less than one unit in the last place of a sum of 35 products.
The Gauss-Newton matrix (exact_hessian = 0) is the oracle's definition: kernel text against oracle only."""
import functools

import numpy as np
import pytest

from oracle import c_oracle
from tests import newton_points as pts
from tests import newton_reference as ref
from tests.emu import emu

H_ = pts.H_
FACTOR = 100.0
CASES = [(N, S) for N in (1, 2, 3) for S in (2, 4, 6)]      # S > 4: the slab layout of p
DELTAS = (0.0, 10.0)


@functools.lru_cache(maxsize=None)
def point(N, S, delta, exact=1):
    """(seed, point): seed 0 where delta > 0 (asserted to factorise), the first seed that factorises at delta = 0"""
    return pts.first_point_that_factorises(N, S, delta, exact, tries=1 if delta > 0 else 32)


@functools.lru_cache(maxsize=None)
def references(N, S, seed):
    """the reference's system of a point, differenced with step 1e-3 and with 2e-3"""
    pt = pts.interior_point(N, S, seed)
    return ref.NewtonReference(*pt, N, S, H_, step=1e-3), ref.NewtonReference(*pt, N, S, H_, step=2e-3)


@functools.lru_cache(maxsize=None)
def measured(N, S, delta):
    """floor and the discrepancies of oracle and one-wave kernel text against the reference, all relative to max |dZ| of the reference"""
    seed, pt = point(N, S, delta)
    r1, r2 = references(N, S, seed)
    dz, dz2 = r1.dz(delta), r2.dz(delta)
    scale = np.abs(dz).max()
    o = c_oracle.debug_qp(*pt, N, S, H_, 1, delta)
    rc, _, _, dze = emu.newton(*pt, delta, N, S, H_)
    assert o["rc"] == 0 and rc == 0
    return dict(seed=seed, scale=scale, spread=pts.sigma_spread(pt[2], pt[3]), floor=np.abs(dz - dz2).max() / scale,
                oracle=np.abs(o["dZ"] - dz).max() / scale, emulator=np.abs(dze - dz).max() / scale)


def measured_lines():
    """the `key = value` lines of the CPU part of profiles/newton_step.txt"""
    out = []
    for N, S in CASES:
        for delta in DELTAS:
            m = measured(N, S, delta)
            out.append(f"N{N}_S{S}_delta{delta:g}: seed = {m['seed']} max_dZ = {m['scale']:.3e} sigma_decades = {m['spread']:.1f} floor = {m['floor']:.3e} "
                       f"bound = {FACTOR * m['floor']:.3e} oracle = {m['oracle']:.3e} emulator = {m['emulator']:.3e}")
    return out


def assert_close_to_oracle(got, want, what):
    """1e-12 relative to max(1, largest entry of the oracle's array) -- module docstring"""
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * max(1.0, np.abs(want).max()), err_msg=what)


@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("N,S", CASES)
def test_oracle_and_kernel_text_match_the_dense_reference_within_the_measured_floor(N, S, delta):
    m = measured(N, S, delta)
    print(f"\nN {N} S {S} delta {delta:g} seed {m['seed']}: max |dZ| {m['scale']:.3e}, floor {m['floor']:.3e}, oracle {m['oracle']:.3e}, emulator {m['emulator']:.3e}")
    assert m["spread"] >= 6.0, m["spread"]
    assert 0 < m["floor"] < 1e-6, m["floor"]      # (the reference resolves its own step: a floor of 1e-6 would make the bound say nothing)
    assert m["oracle"] <= FACTOR * m["floor"], m
    assert m["emulator"] <= FACTOR * m["floor"], m


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("delta", DELTAS)
@pytest.mark.parametrize("N,S", CASES)
def test_kernel_text_direction_and_gains_equal_the_oracle(N, S, delta, exact):
    """dZ, KT, KF of every wave program that has the shape (teams and pairs: S <= 4) against the oracle on the same system, with the exact Hessian
    and with the Gauss-Newton matrix, lanes and waves forward; the team and pair programs equal the one-wave program bit for bit."""
    seed, pt = point(N, S, delta, exact)
    o = c_oracle.debug_qp(*pt, N, S, H_, exact, delta)
    assert o["rc"] == 0
    opts = emu.default_opts(exact_hessian=exact)
    one = None
    for nw in (1,) + ((4, 2, "pair") if S <= 4 else ()):
        rc, kt, kf, dz = emu.newton(*pt, delta, N, S, H_, nw=nw, opts=opts)
        assert rc == 0, nw
        assert_close_to_oracle(kt, o["Kg"], f"KT nw {nw}"); assert_close_to_oracle(kf, o["kff"], f"KF nw {nw}"); assert_close_to_oracle(dz, o["dZ"], f"dZ nw {nw}")
        if one is None:
            one = (kt, kf, dz)
        else:
            assert all(np.array_equal(a, b) for a, b in zip(one, (kt, kf, dz))), nw


def test_regularisation_block_is_where_the_oracle_adds_delta():
    """R of tests/newton_reference.py against the oracle's own maps: riccati() adds delta to the value function on the reduced state s, and the
    oracle's T (dZ = rloc + T s) has a left inverse on the rows R names: S_k T_k = I, so dZ^T R dZ = |s|^2 for every dZ = T s."""
    N, S = 3, 4
    _, pt = point(N, S, 10.0)
    T = c_oracle.debug_qp(*pt, N, S, H_, 1, 10.0)["T"]
    R = ref.regularisation_block(pt[0], pt[1], N, S, H_)
    for k in range(N):
        np.testing.assert_allclose(T[k].T @ R[k * 44:(k + 1) * 44, k * 44:(k + 1) * 44] @ T[k], np.eye(35), atol=1e-12)
