"""Parametric solution sensitivities dx*/dp . dp (include/boundmpc_hip.h bmpc_sens_batch), without a GPU: an independent numpy checker of the
tangent, the kernel text (boundmpc_amd/csrc/bmpc_sens.inl) on the CPU lane emulator against it, the three equations verified at full size, real
solves, the contract cases and the C ABI.

THE CHECKER (dense, numpy.linalg; nothing of the code under test).  Jg and Jh by complex step through oracle/nlp.py; nu by the multiplier map
of tests/multiplier_map.nu_of; LAM from the state columns of the stationarity equation (Jg restricted to the state columns is square
and regular); s and Sigma by the definition.  The system
    H dx + Jg^T dLAM + Jh^T dnu = -r,   Jg dx = -g',   dnu = Sigma (Jh dx + h')
is solved in the null space of Jg: dx = xp + Z y with Jg xp = -g', Z = [I; -Jg_S^-1 Jg_J] (jerk columns J, state columns S), and
    (Z^T H Z + (Jh Z)^T Sigma (Jh Z)) y = -Z^T (r + H xp) - (Jh Z)^T Sigma (Jh xp + h').
Every second derivative of the Lagrangian L = f + LAM . g_eq + nu . h that enters is a MIXED DIRECTIONAL derivative of the scalar L: one direction
by complex step (exact), the other by the five-point central difference with step 1e-3 (truncation h^4 L^(5) / 30, rounding 1e-16 |grad| / h: both
1e-12 of the entries), so a full Hessian (n^2 evaluations) is never formed: Z^T H Z costs (8 N)^2 / 2 pairs, a right-hand side 8 N.

TOLERANCE (measured, not invented; none comes from what the kernel gives).  The checker's tangent is computed twice: with the p-derivative terms
(g', h', Z^T r) by complex step, and by the central difference at the ABI's eps = 1e-6 max(1, |p|_inf) / |dp|_inf.  Their largest discrepancy
relative to max |dx| over the test set is the FLOOR: the noise any differenced right-hand side inherits.  The kernel text must agree with the
complex-step checker within 100 x FLOOR (summation order, and the factorisation of a matrix whose Sigma spans many decades).  The floor is
recomputed here on every run and written to profiles/sensitivity.txt by tests/gpu_sensitivity.py together with the kernel's discrepancy."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import c_oracle, nlp
from tests.multiplier_map import nu_of
from tests import lagrangian as lg
from tests.lagrangian import lagrangian_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NZ, NG, NE, NI, NU = 44, 43, 36, 57, 8
H_ = 0.1
S_ = 4
TOL = 1e-8
MU = TOL * 0.1      # the last barrier level of a solve to TOL (options.tol * options.mu_min_fac)
SENS_LEN = 4
FACTOR = 100.0
PROFILE = os.path.join(ROOT, "profiles", "sensitivity.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sensitivity_checked_set.npz")      # the checked set, for the GPU suite (tests/sensitivity_profile.py)


def abi_eps(p, dp):
    return 1e-6 * max(1.0, np.abs(p).max()) / max(np.abs(dp).max(), 1e-300)


# ---- the problems and the directions ------------------------------------------------------------------------------------------------------
def directions(p, x, N, S, seed):
    """unit steps in q0, dq0, phi0, one weight, one tube coefficient a0 (the first one that moves a tube row at x), phi_max, and a random
    dense dp (name -> dp)"""
    lay, n = nlp.p_layout(S), nlp.n_p(S)
    rng = np.random.default_rng(seed)
    unit = lambda name, i=0: np.eye(n)[lay[name][0] + i]
    dense = rng.normal(size=n) * np.maximum(np.abs(p), 1e-2) * 1e-1
    o, shp = lay["phi_switch"]
    dense[o:o + int(np.prod(shp))] = 0.0      # (segment switches are piecewise-constant conditions: no derivative, as in CasADi)
    ia = next(i for i in range(int(np.prod(lay["a0"][1])))
              if np.any(nlp.internal_ineq(np.asarray(x, complex), p + 1e-30j * unit("a0", i), N, S).imag))
    return {"q0[1]": unit("q0", 1), "dq0[3]": unit("dq0", 3), "phi0": unit("phi0"), "weights[0]": unit("weights"), f"a0[{ia}]": unit("a0", ia),
            "phi_max": unit("phi_max"), "dense": dense}


def small_problems(N, B=3, seed=5):
    """B problems of horizon N solved by the C oracle to TOL (every one must end with status 0; none is left out): B - 1 seeded workload
    problems, and one whose start sits 4 mrad inside a joint limit and moves towards it (the position bound of that joint is active at the
    solution; at N = 3 a tube row as well): (P, X*, lam_g, lam_x)"""
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(B - 1, seed=seed, N=N, workers=1)
    j, v = (3, -0.05) if N == 2 else (5, 0.05)
    q0 = workload.Q0_EXP1.copy()
    q0[j] = np.sign(v) * (nlp.Q_LIM[j] - 0.004)
    pa, xa = workload.pack_cold(q0, N=N)
    pa = pa.copy(); pa[nlp.p_layout(S_)["dq0"][0] + j] = v
    P, X = np.vstack([P, pa[None]]), np.vstack([X, xa[None]])
    r = c_oracle.solve(P, X, N, S_, H_, c_oracle.default_opts(tol=TOL))
    assert (r["status"] == 0).all(), r["status"]
    return P, r["x"], r["lam_g"], r["lam_x"]


def active_rows(p, x, lam_g, lam_x, N, mu=MU, bound_margin=0.0):
    """rows that carry the solution: nu_i s_i within 10 x mu (complementarity at the barrier level) with a multiplier above sqrt(mu) -- at the
    barrier level every row of an interior-point answer has nu s = mu; an ACTIVE one has the small slack"""
    nu, _, _, _, Hv = nu_of(p, x, lam_g, lam_x, N, S_, bound_margin)
    Hv, nu = Hv.reshape(-1), nu.reshape(-1)
    s = np.maximum(-Hv, mu / np.maximum(nu, mu))
    return np.flatnonzero((nu * s <= 10 * mu) & (nu * s >= mu / 10) & (nu > np.sqrt(mu)))


# ---- the checker --------------------------------------------------------------------------------------------------------------------------
def _geq(xc, pc, N, S=S_):
    return lg.g_eq(xc, pc, N, S, H_)


_FD5 = lg.fd5      # five-point central difference of fun(t) at 0, step 1e-3 (tests/lagrangian.py)


class Checker:
    """the system of one point (p, x, lam_g, lam_x, mu); tangent(dp) solves it"""

    def __init__(self, p, x, lam_g, lam_x, N, mu=MU, bound_margin=0.0):
        self.p, self.x, self.N, self.mu = np.asarray(p, float), np.asarray(x, float), N, mu
        n = self.x.size
        nu, _, _, _, Hv = nu_of(p, x, lam_g, lam_x, N, S_, bound_margin)      # (the margin shifts the rows' values, not their derivatives)
        self.nu, self.h = nu.reshape(-1), Hv.reshape(-1)
        gf, self.Jg, self.Jh = lg.jacobians(self.p, self.x, N, S_, H_)
        self.J, self.S = lg.column_split(n)
        self.lam = lg.lam_from_state_columns(gf, self.Jg, self.Jh, self.nu)
        self.s = np.maximum(-self.h, mu / np.maximum(self.nu, mu))
        self.Sigma = self.nu / self.s
        self.Z, self.JgS = lg.null_space(self.Jg)
        Z = self.Z
        # Z^T H Z: complex step along Z_a, five-point difference along Z_b (upper triangle)
        Hzz = lg.reduced_hessian(self.x, self.p, self.lam, self.nu, Z, N, S_, H_)
        JhZ = self.Jh @ Z
        self.K = Hzz + JhZ.T @ (self.Sigma[:, None] * JhZ)
        self.JhZ = JhZ

    def _L(self, xc, pc):
        return lg.lagrangian(xc, pc, self.lam, self.nu, self.N, S_, H_)

    def _grad_along(self, x, p, U):
        """U^T grad_x L at (x, p) by complex step, one evaluation per column"""
        return lg.grad_along(x, p, self.lam, self.nu, U, self.N, S_, H_)

    def tangent(self, dp, central=False):
        """dx (and dnu) along dp; central: the p-derivative terms by the central difference at the ABI's eps instead of the complex step"""
        N, p, x, Z = self.N, self.p, self.x, self.Z
        if not np.any(dp):
            return np.zeros(x.size), np.zeros(self.nu.size)
        if central:
            e = abi_eps(p, dp)
            ddt = lambda fun: (fun(p + e * dp) - fun(p - e * dp)) / (2 * e)
        else:
            ddt = lambda fun: fun(p + 1e-30j * dp).imag / 1e-30
        gd = ddt(lambda pc: _geq(x.astype(pc.dtype), pc, N))
        hd = ddt(lambda pc: nlp.internal_ineq(x.astype(pc.dtype), pc, N, S_))
        xp = np.zeros(x.size); xp[self.S] = np.linalg.solve(self.JgS, -gd)
        # Z^T r = d/dt Z^T grad_x L(x; p + t dp)
        if central:
            Zr = ddt(lambda pc: self._grad_along(x, pc, Z))
        else:
            Zr = _FD5(lambda t: np.array([self._L(x + t * Z[:, a], p + 1e-30j * dp).imag / 1e-30 for a in range(Z.shape[1])]))
        ZHxp = _FD5(lambda t: self._grad_along(x + t * xp, p, Z)) if np.any(xp) else np.zeros(Z.shape[1])
        rhs = -(Zr + ZHxp) - self.JhZ.T @ (self.Sigma * (self.Jh @ xp + hd))
        y = np.linalg.solve(self.K, rhs)
        dx = xp + Z @ y
        return dx, self.Sigma * (self.Jh @ dx + hd)


# ---- the kernel text on the CPU lane emulator (tests/emu/bmpc_emu_sens.cpp) ----
def _emu():
    from tests.emu import emu
    return emu.service_lib("sens")


def emu_sens(p, x, dp, lam_g, lam_x, N, S=S_, mu=MU, lane_order=0, poison=True, want=True, opts=None):
    from tests.emu import emu
    o = opts if opts is not None else emu.default_opts()
    p, x, dp = (np.ascontiguousarray(np.atleast_2d(a), dtype=float) for a in (p, x, dp))
    B = p.shape[0]
    arr = lambda a: None if a is None else np.ascontiguousarray(np.atleast_2d(a), dtype=float)
    lg, lx = arr(lam_g), arr(lam_x)
    out = dict(dx=np.full((B, N * NZ), -7.0), rec=np.full((B, SENS_LEN), -7.0))
    if want:
        out.update(dlam_eq=np.full((B, N * NE), -7.0), dnu=np.full((B, N * NI), -7.0))
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = _emu().bmpc_emu_sens(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(H_), ctypes.byref(o), ctypes.c_int(B), vp(p), vp(x), vp(lg), vp(lx), vp(dp),
                              ctypes.c_double(mu), vp(out["dx"]), vp(out.get("dlam_eq")), vp(out.get("dnu")), vp(out["rec"]), ctypes.c_int(lane_order),
                              ctypes.c_int(int(poison)))
    assert rc == 0
    return out


# ---- 1., 2. the independent checker, its floor, the emulated kernel text ------------------------------------------------------------------
_CACHE = {}


def checked_set():
    """The test set of items 1 and 2: per horizon (2, 3) the problems, per problem and direction the checker's tangent twice.
    Returns a list of dicts (N, b, name, p, x, lam_g, lam_x, dp, dx, dx_central)."""
    if "set" in _CACHE:
        return _CACHE["set"]
    rows = []
    for N, B in ((2, 3), (3, 2)):
        P, X, LG, LX = small_problems(N, B)
        for b in range(B):
            ck = Checker(P[b], X[b], LG[b], LX[b], N)
            for name, dp in directions(P[b], X[b], N, S_, seed=10 * N + b).items():
                dx, _ = ck.tangent(dp)
                dxc, _ = ck.tangent(dp, central=True)
                rows.append(dict(N=N, b=b, name=name, p=P[b], x=X[b], lam_g=LG[b], lam_x=LX[b], dp=dp, dx=dx, dx_central=dxc))
    _CACHE["set"] = rows
    return rows


def _scale(r):
    return max(np.abs(r["dx"]).max(), 1e-300)


def floor_of(rows):
    return max(np.abs(r["dx"] - r["dx_central"]).max() / _scale(r) for r in rows)


def discrepancy_of(rows, fn):
    """largest |fn(row) - checker dx| / max |dx| over the set"""
    return max(np.abs(fn(r) - r["dx"]).max() / _scale(r) for r in rows)


def measured_lines():
    rows = checked_set()
    fl = floor_of(rows)
    de = discrepancy_of(rows, lambda r: emu_sens(r["p"], r["x"], r["dp"], r["lam_g"], r["lam_x"], r["N"])["dx"][0])
    return [f"checked_points = {len(rows)}", f"floor = {fl:.6e}", f"bound = {FACTOR * fl:.6e}", f"emulator_discrepancy = {de:.6e}"]


def pack_rows(rows):
    """the checked set as arrays (rows padded to the longest horizon's lengths; n = 44 N entries of x / dx are valid)"""
    n = max(r["x"].size for r in rows)
    pad = lambda a, m: np.concatenate([a, np.zeros(m - a.size)])
    out = dict(N=np.array([r["N"] for r in rows]), b=np.array([r["b"] for r in rows]), name=np.array([r["name"] for r in rows]))
    for k, m in (("p", rows[0]["p"].size), ("dp", rows[0]["p"].size), ("x", n), ("lam_x", n), ("dx", n), ("dx_central", n), ("lam_g", n)):
        out[k] = np.stack([pad(r[k], m) for r in rows])
    return out


def unpack_rows(d):
    rows = []
    for i, N in enumerate(d["N"]):
        N = int(N)
        r = dict(N=N, b=int(d["b"][i]), name=str(d["name"][i]), p=d["p"][i], dp=d["dp"][i])
        for k, m in (("x", N * NZ), ("lam_x", N * NZ), ("dx", N * NZ), ("dx_central", N * NZ), ("lam_g", N * NG)):
            r[k] = np.ascontiguousarray(d[k][i][:m])
        rows.append(r)
    return rows


def golden_rows():
    return unpack_rows(np.load(GOLDEN))


def test_golden_checked_set_is_what_the_checker_computes():
    """the file the GPU suite reads holds this checker's inputs and tangents (the tangents up to the rounding of numpy.linalg on another machine:
    1e-3 of the floor's own bound)"""
    rows, gold = checked_set(), golden_rows()
    assert len(rows) == len(gold)
    fl = floor_of(rows)
    for r, g in zip(rows, gold):
        assert (r["N"], r["b"], r["name"]) == (g["N"], g["b"], g["name"])
        for k in ("p", "dp", "x", "lam_g", "lam_x"):
            np.testing.assert_allclose(g[k], r[k], rtol=1e-9, atol=1e-12, err_msg=k)
        for k in ("dx", "dx_central"):
            assert np.abs(g[k] - r[k]).max() <= 0.1 * FACTOR * fl * _scale(r), k


def test_problem_set_has_an_active_and_an_inactive_problem():
    """item 1: every oracle solve ends with status 0 (small_problems asserts it: no problem is left out); at least one problem has an active tube
    row or joint bound, at least one has none"""
    counts = []
    for N, B in ((2, 3), (3, 2)):
        P, X, LG, LX = small_problems(N, B)
        for b in range(B):
            act = active_rows(P[b], X[b], LG[b], LX[b], N) % NI
            counts.append(int(((act >= 16) & (act != 44) & (act != 45) & (act != 46)).sum()))      # joint bounds (q, dq) and tube rows
    print("active joint-bound / tube rows per problem:", counts)
    assert max(counts) > 0 and min(counts) == 0, counts


def test_emulated_kernel_matches_the_checker_within_the_measured_floor():
    rows = checked_set()
    fl = floor_of(rows)
    print(f"floor (complex step vs central difference at the ABI's eps, relative to max |dx|) = {fl:.3e}; bound = {FACTOR * fl:.3e}")
    assert 0 < fl < 1e-4, fl      # (a floor of 1e-4 would mean the checker itself is broken)
    worst = 0.0
    for r in rows:
        o = emu_sens(r["p"], r["x"], r["dp"], r["lam_g"], r["lam_x"], r["N"])
        assert o["rec"][0, 0] == 0.0, (r["N"], r["b"], r["name"], o["rec"][0])
        e = np.abs(o["dx"][0] - r["dx"]).max() / _scale(r)
        print(f"  N={r['N']} problem {r['b']} {r['name']:<11} max|dx| {np.abs(r['dx']).max():.3e}  checker twice {np.abs(r['dx'] - r['dx_central']).max() / _scale(r):.2e}  kernel text {e:.2e}")
        worst = max(worst, e)
    print(f"worst kernel-text discrepancy = {worst:.3e}")
    assert worst <= FACTOR * fl, (worst, fl)


# ---- 3. full size, no dense solve: the three equations verified directly --------------------------------------------------------------------
def full_size_points(B=2, seed=2, tol=TOL):
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(B, seed=seed, N=10, workers=1)
    r = c_oracle.solve(P, X, 10, S_, H_, c_oracle.default_opts(tol=tol))
    assert (r["status"] == 0).all(), r["status"]
    return P, r["x"], r["lam_g"], r["lam_x"]


def equation_residuals(p, x, lam_g, lam_x, dp, dx, dlam, dnu, N, mu=MU, S=S_, stationarity=True, bound_margin=0.0):
    """(residual, scale of the terms that cancel in it) of the three equations at one point, by complex step through oracle/nlp.py; the
    stationarity row by a central difference of the complex-step Lagrangian gradient (test_kkt_certificate.lagrangian_gradient)."""
    nu, _, _, _, Hv = nu_of(p, x, lam_g, lam_x, N, S, bound_margin)
    nu, hv = nu.reshape(-1), Hv.reshape(-1)
    lam = c_oracle.adjoint(p, x, nu, N, S, H_)[0]
    Sigma = nu / np.maximum(-hv, mu / np.maximum(nu, mu))
    xc, pc = x + 1e-30j * dx, p + 1e-30j * dp
    a, b = _geq(xc, p.astype(complex), N, S).imag / 1e-30, _geq(x.astype(complex), pc, N, S).imag / 1e-30
    res = dict(eq=(np.abs(a + b).max(), max(np.abs(a).max(), np.abs(b).max())))
    a, b = nlp.internal_ineq(xc, p.astype(complex), N, S).imag / 1e-30, nlp.internal_ineq(x.astype(complex), pc, N, S).imag / 1e-30
    res["row"] = (np.abs(dnu - Sigma * (a + b)) / np.maximum(Sigma, 1e-300)).max(), max(np.abs(a).max(), np.abs(b).max())      # (per unit of Sigma)
    if stationarity:
        t = 1e-6 * max(1.0, np.abs(x).max(), np.abs(p).max()) / max(np.abs(dx).max(), np.abs(dp).max())
        gp = lagrangian_gradient(p + t * dp, x + t * dx, lam + t * dlam, nu + t * dnu, N, S)
        gm = lagrangian_gradient(p - t * dp, x - t * dx, lam - t * dlam, nu - t * dnu, N, S)
        mult = lagrangian_gradient(p, x, dlam, dnu, N, S) - lagrangian_gradient(p, x, 0 * dlam, 0 * dnu, N, S)      # Jg^T dLAM + Jh^T dnu
        res["stat"] = (np.abs(gp - gm).max() / (2 * t), np.abs(mult).max())
    return res


def test_full_size_tangent_satisfies_the_three_equations():
    """item 3 at N = 10, S = 4 on oracle-converged workload problems.  Tolerance by the rule of item 2: FACTOR x floor, relative to the largest of
    the terms that cancel in the equation (Jg dx against g'; Jh dx against h', per unit of Sigma; the multiplier terms Jg^T dLAM + Jh^T dnu against
    H dx + r)."""
    fl = floor_of(checked_set())
    P, X, LG, LX = full_size_points()
    for b, name in ((0, "q0[1]"), (1, "dense")):
        dp = directions(P[b], X[b], 10, S_, seed=b)[name]
        o = emu_sens(P[b], X[b], dp, LG[b], LX[b], 10)
        assert o["rec"][0, 0] == 0.0
        res = equation_residuals(P[b], X[b], LG[b], LX[b], dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], 10)
        for k, (r, sc) in res.items():
            print(f"  N=10 problem {b} {name}: {k} residual {r:.3e} scale {sc:.3e} ratio {r / sc:.3e} (bound {FACTOR * fl:.3e})")
            assert r <= FACTOR * fl * sc, (b, name, k, r, sc)


# ---- 4. against real solves (sanity, loose) ------------------------------------------------------------------------------------------------
def real_solve_comparison(fn, tol=1e-10):
    """x*(p + t dp) - x*(p - t dp) over 2 t from oracle solves at tolerance 1e-10 for three t (the active set must not change: the multiplier
    pattern is compared), against fn(p, x, lam_g, lam_x, dp, mu) -> dx.  Returns (cosine, relative size error, spread of the finite difference)."""
    P, X, LG, LX = full_size_points(B=1, seed=4, tol=tol)
    p, o = P[0], c_oracle.default_opts(tol=tol)
    dp = directions(p, X[0], 10, S_, seed=0)["q0[1]"]
    fd, act = [], []
    for t in (1e-4, 2e-4, 4e-4):
        rp = c_oracle.solve(p + t * dp, X[0], 10, S_, H_, o); rm = c_oracle.solve(p - t * dp, X[0], 10, S_, H_, o)
        assert rp["status"][0] == 0 and rm["status"][0] == 0
        fd.append((rp["x"][0] - rm["x"][0]) / (2 * t))
        act += [tuple(active_rows(q, r["x"][0], r["lam_g"][0], r["lam_x"][0], 10, mu=tol * 0.1)) for q, r in ((p + t * dp, rp), (p - t * dp, rm))]
    assert len(set(act)) == 1, "the active set changed over the finite difference"
    dx = fn(p, X[0], LG[0], LX[0], dp, tol * 0.1)
    mid = fd[1]
    spread = max(np.linalg.norm(f - mid) for f in fd) / np.linalg.norm(mid)
    cos = dx @ mid / (np.linalg.norm(dx) * np.linalg.norm(mid))
    size = abs(np.linalg.norm(dx) - np.linalg.norm(mid)) / np.linalg.norm(mid)
    return cos, size, spread


def test_tangent_agrees_with_differenced_real_solves():
    cos, size, spread = real_solve_comparison(lambda p, x, lg, lx, dp, mu: emu_sens(p, x, dp, lg, lx, 10, mu=mu)["dx"][0])
    print(f"cosine {cos:.9f}; size error {size:.3e}; spread of the finite difference over t = 1e-4, 2e-4, 4e-4: {spread:.3e}")
    assert cos >= 0.99
    assert size <= spread, (size, spread)


# ---- 5. contract cases on the emulated kernel text ------------------------------------------------------------------------------------------
def _point(N=3):
    P, X, LG, LX = small_problems(N, 2)
    return P[1], X[1], LG[1], LX[1]


def test_zero_direction_gives_exactly_zero_and_status_0():
    p, x, lg, lx = _point()
    o = emu_sens(p, x, np.zeros_like(p), lg, lx, 3)
    assert (o["dx"] == 0).all() and (o["dlam_eq"] == 0).all() and (o["dnu"] == 0).all()
    assert o["rec"][0, 0] == 0 and o["rec"][0, 2] == 0 and o["rec"][0, 3] == 0


def test_tangent_is_linear_in_the_direction_within_the_floor():
    fl = floor_of(checked_set())
    p, x, lg, lx = _point()
    d = directions(p, x, 3, S_, seed=1)
    d1, d2 = d["q0[1]"], d["dense"]
    f = lambda dp: emu_sens(p, x, dp, lg, lx, 3)["dx"][0]
    a, b, a2, ab = f(d1), f(d2), f(2 * d1), f(d1 + d2)
    assert np.abs(a2 - 2 * a).max() <= fl * np.abs(a2).max()
    assert np.abs(ab - (a + b)).max() <= fl * max(np.abs(a).max(), np.abs(b).max())


def test_null_multipliers_equal_explicit_zeros_bit_for_bit():
    p, x, _, _ = _point()
    dp = directions(p, x, 3, S_, seed=1)["dense"]
    a = emu_sens(p, x, dp, None, None, 3)
    b = emu_sens(p, x, dp, np.zeros(3 * NG), np.zeros(3 * NZ), 3)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_non_finite_input_gives_status_3_and_nan_never_a_fault():
    p, x, lg, lx = _point()
    dp = directions(p, x, 3, S_, seed=1)["dense"]
    for which, bad in (("x", np.nan), ("x", np.inf), ("p", np.nan), ("dp", -np.inf), ("dp", np.nan)):
        a = dict(x=x.copy(), p=p.copy(), dp=dp.copy())
        a[which][7] = bad
        o = emu_sens(a["p"], a["x"], a["dp"], lg, lx, 3)
        assert o["rec"][0, 0] == 3.0 and np.isnan(o["dx"]).all() and np.isnan(o["dlam_eq"]).all() and np.isnan(o["dnu"]).all(), (which, bad)
    lgn = lg.copy(); lgn[40] = np.nan      # a non-finite multiplier counts as 0 (the map's rule)
    lgz = lg.copy(); lgz[40] = 0.0
    assert emu_sens(p, x, dp, lgn, lx, 3)["dx"].tobytes() == emu_sens(p, x, dp, lgz, lx, 3)["dx"].tobytes()


def regularised_point(N=3):
    """a point whose exact Hessian is indefinite on the null space of Jg: away from the solution, with large random equality-consistent multipliers
    on the tube rows only (the tube rows' own curvature c'' enters with either sign)"""
    p, x, lg, lx = _point(N)
    rng = np.random.default_rng(11)
    xp = x + rng.normal(size=x.size) * 0.05
    xp.reshape(N, NZ)[:, 41] = np.abs(xp.reshape(N, NZ)[:, 41]) + 0.3
    lgp = np.zeros(N * NG); lgp.reshape(N, NG)[:, 38:] = 1e4
    return p, xp, lgp, None


def test_a_point_that_needs_regularisation_reports_status_1_with_delta():
    p, x, lg, lx = regularised_point()
    dp = directions(p, x, 3, S_, seed=1)["q0[1]"]
    o = emu_sens(p, x, dp, lg, lx, 3, mu=1e-2)
    print("record:", o["rec"][0])
    assert o["rec"][0, 0] == 1.0 and o["rec"][0, 1] > 0 and np.isfinite(o["dx"]).all()


def test_emulated_runs_are_bitwise_deterministic_in_any_lane_order():
    p, x, lg, lx = _point()
    dp = directions(p, x, 3, S_, seed=1)["dense"]
    ref = emu_sens(p, x, dp, lg, lx, 3)
    for order, poison in ((0, False), (1, True), (2, True)):
        o = emu_sens(p, x, dp, lg, lx, 3, lane_order=order, poison=poison)
        for k in ref:
            assert o[k].tobytes() == ref[k].tobytes(), (order, k)


def other_instantiation_point(N, S):
    """an oracle-converged workload problem of a size that runs wave_sensitivity<false> (S > 4 or N > 11: iterate and direction in the workspace)
    and the unit direction q0[1]"""
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(1, seed=3, N=N, S=S, workers=1)
    r = c_oracle.solve(P, X, N, S, H_, c_oracle.default_opts(tol=TOL))
    assert r["status"][0] == 0
    dp = np.eye(nlp.n_p(S))[nlp.p_layout(S)["q0"][0] + 1]
    return P[0], r["x"][0], r["lam_g"][0], r["lam_x"][0], dp


@pytest.mark.parametrize("N,S", [(4, 5), (12, 4)])
def test_instantiation_without_the_lds_iterate_satisfies_the_equations(N, S):
    """S > 4 and N > 11 run wave_sensitivity<false>: its tangent satisfies the equations like the other's (all three at S = 5; at N = 12 the
    equality rows and the row equation: the stationarity check costs five complex-step gradients of 528 evaluations there).  Bound: the rule of item 2."""
    fl = floor_of(checked_set())
    p, x, lg, lx, dp = other_instantiation_point(N, S)
    o = emu_sens(p, x, dp, lg, lx, N, S=S)
    assert o["rec"][0, 0] == 0.0
    res = equation_residuals(p, x, lg, lx, dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], N, S=S, stationarity=N < 10)
    assert ("stat" in res) == (N < 10)
    for k, (r, sc) in res.items():
        print(f"  N={N} S={S}: {k} residual {r:.3e} scale {sc:.3e} ratio {r / sc:.3e} (bound {FACTOR * fl:.3e})")
        assert r <= FACTOR * fl * sc, (N, S, k, r, sc)


# ---- 6. C ABI and the Python argument checks ------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_the_entry_points():
    from boundmpc_amd import _lib, build, solver
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "boundmpc_hip.h")).read(), flags=re.S)
    assert re.search(r"int bmpc_sens_len\(void\);", hdr)
    assert re.search(r"int bmpc_sens_batch\(bmpc_handle \*h, int B, const double \*p, const double \*x, const double \*lam_g, const double \*lam_x, const double \*dp,"
                     r"\s*double mu,\s*double \*dx, double \*dlam_eq, double \*dnu, double \*rec, void \*hip_stream\);", hdr)
    assert re.search(r"int bmpc_sens_batch_host\(bmpc_handle \*h, int B, const double \*p, const double \*x, const double \*lam_g, const double \*lam_x, const double \*dp,"
                     r"\s*double mu,\s*double \*dx, double \*dlam_eq, double \*dnu, double \*rec\);", hdr)
    slots = dict(re.findall(r"BMPC_SENS_(\w+) = (\d+)", hdr))
    assert [int(slots[k]) for k in ("STATUS", "DELTA", "RHS", "DX", "LEN")] == [0, 1, 2, 3, 4]
    assert (solver.SENS_STATUS, solver.SENS_DELTA, solver.SENS_RHS, solver.SENS_DX) == (0, 1, 2, 3) and len(solver.SENS_FIELDS) == SENS_LEN
    assert _emu().bmpc_emu_sens_len() == SENS_LEN
    assert os.path.join(build.CSRC, "bmpc_sens.inl") in build.SOURCES
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("bmpc_sens_len", "bmpc_sens_batch", "bmpc_sens_batch_host"):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert lib.bmpc_sens_len() == SENS_LEN
    # argument checks that need no device: a NULL handle / buffers, B < 1
    vp, cd = ctypes.c_void_p, ctypes.c_double
    lib.bmpc_sens_batch.argtypes = [vp, ctypes.c_int] + [vp] * 5 + [cd] + [vp] * 5
    lib.bmpc_sens_batch_host.argtypes = [vp, ctypes.c_int] + [vp] * 5 + [cd] + [vp] * 4
    assert lib.bmpc_sens_batch(None, 1, None, None, None, None, None, 0.0, None, None, None, None, None) == 1
    assert lib.bmpc_sens_batch_host(None, 0, None, None, None, None, None, 0.0, None, None, None, None) == 1


class _FakeLib:
    def __getattr__(self, n):
        raise AssertionError(f"{n}: the argument check must raise before the library is called")


def test_python_argument_checks_raise():
    from boundmpc_amd.solver import BatchedOCPSolver, NlpSolverShim
    s = BatchedOCPSolver.__new__(BatchedOCPSolver)
    s.N, s.S, s.n_w, s.n_g, s.n_p, s._lib, s._h = 10, 4, 440, 430, 505, _FakeLib(), None
    with pytest.raises(ValueError, match="shape mismatch"):
        s.sensitivity_host(np.zeros((2, 505)), np.zeros((2, 440)), np.zeros((2, 504)))
    with pytest.raises(ValueError, match="shape mismatch"):
        s.sensitivity_host(np.zeros((2, 505)), np.zeros((2, 440)), np.zeros((3, 2, 505)))
    with pytest.raises(ValueError, match="lam_g has shape"):
        s.sensitivity_host(np.zeros((2, 505)), np.zeros((2, 440)), np.zeros((2, 505)), lam_g=np.zeros((2, 440)))
    with pytest.raises(ValueError, match="float64 tensors on the GPU"):
        import torch
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64)
        s.sensitivity(z(2, 505), z(2, 440), z(2, 505))
    shim = NlpSolverShim.__new__(NlpSolverShim)
    shim._s = s
    with pytest.raises(RuntimeError, match="previous solver"):
        shim.sensitivity(np.zeros(505))


def test_profile_states_the_floor_and_the_kernel_discrepancy():
    """profiles/sensitivity.txt states the floor, the bound and the discrepancy of the kernel text (CPU part: tests/sensitivity_profile.py), and a
    discrepancy it states -- the emulator's, the GPU's once tests/gpu_sensitivity.py has been run -- is inside the bound it states"""
    text = open(PROFILE).read()
    val = lambda key: re.search(rf"^{key} = (\S+)$", text, re.M)
    for key in ("floor", "bound", "emulator_discrepancy"):
        assert val(key), key
    assert float(val("bound").group(1)) == pytest.approx(FACTOR * float(val("floor").group(1)), rel=1e-5)
    for key in ("emulator_discrepancy", "gpu_discrepancy"):
        if val(key):
            assert float(val(key).group(1)) <= float(val("bound").group(1)), key
