"""KKT certificate of any primal-dual point (include/boundmpc_hip.h bmpc_kkt_batch), without a GPU: an independent numpy checker of the record
(oracle/nlp.py values, the multiplier map of tests/multiplier_map.py, the C oracle's adjoint, and -- independently of that adjoint -- a complex-step gradient of the
Lagrangian), the kernel text (boundmpc_amd/csrc/bmpc_kkt.inl) on the CPU lane emulator against it, the ordering "solution below cold start", the
gap rules and the C ABI.

Tolerances (none comes from what the kernel gives).  `dual` and `lam_eq_gap` are entries of the adjoint's outputs: 1e-11 max(1, max |LAM|), the
bound of test_oracle_golden.test_c_oracle_adjoint_is_lagrangian_gradient.  Everything else is 1e-12 RELATIVE TO THE TERMS THE VALUE IS FORMED
FROM: f relative to |f| (test_oracle_golden: 1e-12 |f|); a residual g or h is a difference of O(1) terms whose two evaluations agree to 1e-13
absolute (test_oracle_golden's atol for g), so prim_eq / prim_ineq get 1e-13 + 1e-12 |value|; a converted multiplier carries 1e-12 (nu + lam (|c| +
wd)) (test_dual_warm_start.assert_state_close), which compl inherits times the row's slack and the re-exported tube multiplier divided by 2 wd.  A
tolerance relative to the VALUE of a residual would be unattainable for any two codes: at the reference's cold start |g| is 1e-15 of rounding."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import c_oracle, nlp
from tests.lagrangian import lagrangian_gradient
from tests.multiplier_map import export_of, nu_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
NZ, NG, NE, NI, NU = 44, 43, 36, 57, 8
FIELDS = ("E", "dual", "prim_eq", "prim_ineq", "compl", "lam_eq_gap", "lam_ineq_gap", "f")
PROFILE = os.path.join(ROOT, "profiles", "kkt_certificate.txt")


# ---- the record in numpy -------------------------------------------------------------------------------------------------------------------
def _gap(given, own):
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(np.asarray(given, dtype=float) - own)
    return np.where(np.isfinite(d), d, np.inf)


def checker(p, x, lam_g, lam_x, N, S, h=0.1, bound_margin=0.0):
    """One problem (bound_margin: the handle's options.bound_margin, which tightens the joint rows of h).  Returns (record dict, tolerance dict, extras dict with g, lam_g (consistent), rj, nu)."""
    p, x = np.asarray(p, dtype=float), np.asarray(x, dtype=float)
    f, g = nlp.nlp_eval(x, p, N, S, h)
    g2 = g.reshape(N, NG)
    nu, sc, c, wd, H = nu_of(p, x, lam_g, lam_x, N, S, bound_margin)
    lam, rj, _ = c_oracle.adjoint(p, x, nu.ravel(), N, S, h)
    lam = lam.reshape(N, NE)
    slack, viol = np.maximum(-H, 0.0), np.maximum(H, 0.0)
    rec = dict(dual=np.abs(rj).max(), prim_eq=np.abs(g2[:, :NE]).max(), prim_ineq=viol.max(), compl=(nu * slack).max(), f=float(f))
    sl, sn = np.abs(lam).sum(), nu.sum()
    sd, scl = max(100.0, (sl + sn) / (N * (NE + NI))) / 100.0, max(100.0, sn / (N * NI)) / 100.0
    rec["E"] = max(rec["dual"] / sd, max(rec["prim_eq"], rec["prim_ineq"]), rec["compl"] / scl)
    lg_out, lx_out = export_of(nu, wd)
    rec["lam_eq_gap"] = 0.0 if lam_g is None else float(_gap(np.asarray(lam_g).reshape(N, NG)[:, :NE], lam).max())
    gi = 0.0
    if lam_g is not None:
        gi = max(gi, float(_gap(np.asarray(lam_g).reshape(N, NG)[:, NE:], lg_out).max()))
    if lam_x is not None:
        gi = max(gi, float(_gap(np.asarray(lam_x).reshape(N, NZ), lx_out).max()))
    rec["lam_ineq_gap"] = gi
    scale = max(1.0, np.abs(lam).max())
    with np.errstate(invalid="ignore", divide="ignore"):
        tube = np.nan_to_num(np.where(wd > 0, sc[:, 47::2] / wd, 0.0)).max()
    tol = dict(dual=1e-11 * scale, lam_eq_gap=1e-11 * scale, f=1e-12 * abs(f),
               prim_eq=1e-13 + 1e-12 * rec["prim_eq"], prim_ineq=1e-13 + 1e-12 * rec["prim_ineq"],
               compl=1e-12 * (rec["compl"] + (sc * slack).max()) + 1e-13 * nu.max(),
               lam_ineq_gap=1e-12 * (rec["lam_ineq_gap"] + tube + nu.max()) if np.isfinite(rec["lam_ineq_gap"]) else 0.0)
    tol["E"] = max(tol["dual"] / sd, tol["prim_eq"], tol["prim_ineq"], tol["compl"] / scl) + 1e-12 * rec["E"]
    lam_g_out = np.concatenate([lam, lg_out], axis=1).ravel()
    return rec, tol, dict(g=g, lam_g=lam_g_out, rj=rj, nu=nu, scale=scale, tube=tube)


def assert_record(got, rec, tol, what=""):
    for i, k in enumerate(FIELDS):
        if np.isinf(rec[k]):
            assert got[i] == rec[k], (what, k, got[i])
        else:
            assert abs(got[i] - rec[k]) <= tol[k], (what, k, got[i], rec[k], tol[k])


# ---- the kernel text on the CPU lane emulator (tests/emu/bmpc_emu_kkt.cpp) ----
def _emu():
    from tests.emu import emu
    return emu.service_lib("kkt")


def emu_cert(p, x, lam_g, lam_x, N, S, lane_order=0, poison=True, want=True, bound_margin=0.0):
    from tests.emu import emu
    o = emu.default_opts(bound_margin=bound_margin)
    p, x = np.ascontiguousarray(np.atleast_2d(p), dtype=float), np.ascontiguousarray(np.atleast_2d(x), dtype=float)
    B = p.shape[0]
    arr = lambda a: None if a is None else np.ascontiguousarray(np.atleast_2d(a), dtype=float)
    lg, lx = arr(lam_g), arr(lam_x)
    out = dict(cert=np.full((B, 8), -7.0))
    if want:
        out.update(g=np.full((B, N * NG), -7.0), lam_g=np.full((B, N * NG), -7.0), rj=np.full((B, N * NU), -7.0))
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = _emu().bmpc_emu_kkt(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(0.1), ctypes.byref(o), ctypes.c_int(B), vp(p), vp(x), vp(lg), vp(lx),
                             vp(out["cert"]), vp(out.get("g")), vp(out.get("lam_g")), vp(out.get("rj")), ctypes.c_int(lane_order), ctypes.c_int(int(poison)))
    assert rc == 0
    return out


def assert_extras(out, b, ex, N):
    """the optional outputs of problem b against the checker's: g (1e-13, test_oracle_golden), the consistent multipliers and rj (the adjoint's bound)"""
    np.testing.assert_allclose(out["g"][b], ex["g"], rtol=1e-12, atol=1e-13)
    got, want = out["lam_g"][b].reshape(N, NG), ex["lam_g"].reshape(N, NG)
    np.testing.assert_allclose(got[:, :NE], want[:, :NE], rtol=0, atol=1e-11 * ex["scale"])
    np.testing.assert_allclose(got[:, NE:], want[:, NE:], rtol=1e-12, atol=1e-12 * (ex["tube"] + ex["nu"].max()))
    np.testing.assert_allclose(out["rj"][b], ex["rj"], rtol=0, atol=1e-11 * ex["scale"])


def _g6(which):
    d = np.load(os.path.join(G, f"g6_pack_exp{which}_tick0.npz"))
    return d["p_f64"], d["x0_f64"]


def fixture_problems():
    """The g6 tick-0 problems of both experiments, the G7 ticks of both and a 64-problem sample of BASELINE configs[1] (seed-0 batch)."""
    from boundmpc_amd import workload
    d1, d2 = np.load(os.path.join(G, "g7_closedloop_exp1.npz")), np.load(os.path.join(G, "g7_closedloop_exp2.npz"))
    P, X, _ = workload.make_batch(64, seed=0, workers=1)
    g6 = [_g6(1), _g6(2)]
    return (np.concatenate([np.stack([a[0] for a in g6]), d1["p"], d2["p"], P]), np.concatenate([np.stack([a[1] for a in g6]), d1["x0"], d2["x0"], X]))


@pytest.fixture(scope="module")
def solved():
    P, X = fixture_problems()
    r = c_oracle.solve(P, X, 10, 4, 0.1, c_oracle.default_opts(tol=1e-8), nthreads=8)
    return P, X, r


def certify_oracle_solutions(P, X, r, N=10, S=4):
    """numpy records of the oracle's solutions (with its multipliers) and of its cold starts (no multipliers), converged problems only."""
    ok = np.flatnonzero(r["status"] == 0)
    at_sol = [checker(P[b], r["x"][b], r["lam_g"][b], r["lam_x"][b], N, S) for b in ok]
    at_x0 = [checker(P[b], X[b], None, None, N, S) for b in ok]
    return ok, at_sol, at_x0


def measured_lines(P, X, r, tol=1e-8):
    ok, at_sol, _ = certify_oracle_solutions(P, X, r)
    E = np.array([c[0]["E"] for c in at_sol])
    return ok, E, [f"problems = {len(r['status'])} (converged: {len(ok)})", f"tol = {tol:g}", f"max_E = {E.max():.6e}", f"max_E_over_tol = {E.max() / tol:.6f}",
                   f"median_E_over_tol = {np.median(E) / tol:.6f}", f"max_E_over_kkt_of_the_solve = {(E / r['kkt'][ok]).max():.6f}",
                   f"median_E_over_kkt_of_the_solve = {np.median(E / r['kkt'][ok]):.6f}"]


def test_checker_multipliers_zero_the_state_gradient_and_rj_is_the_jerk_gradient():
    """The independent leg: with the KERNEL's returned lam_g (equality rows) the complex-step gradient of f + lam_eq . g_eq + nu . h vanishes in every
    state variable and equals the kernel's rj in the jerks -- at a converged solution with its multipliers, at a cold start without, at a perturbed
    point with random multipliers.  Bound: test_c_oracle_adjoint_is_lagrangian_gradient's 1e-11 max(1, max |lam|)."""
    rng = np.random.default_rng(3)
    for which in (1, 2):
        p, x0 = _g6(which)
        r = c_oracle.solve(p, x0, 10, 4, 0.1, c_oracle.default_opts(tol=1e-8))
        xp = x0 + rng.normal(size=x0.shape) * 0.02
        xp.reshape(10, NZ)[:, 41] = np.abs(xp.reshape(10, NZ)[:, 41]) + np.linspace(0.1, 2.0, 10)
        cases = [(r["x"][0], r["lam_g"][0], r["lam_x"][0]), (x0, None, None)]
        if which == 1:
            cases.append((xp, rng.normal(size=430), rng.normal(size=440)))
        for x, lg, lx in cases:
            out = emu_cert(p, x, lg, lx, 10, 4)
            nu = nu_of(p, x, lg, lx, 10, 4)[0]
            lam_eq = out["lam_g"][0].reshape(10, NG)[:, :NE]
            gl = lagrangian_gradient(p, x, lam_eq, nu, 10, 4)
            scale = max(1.0, np.abs(lam_eq).max())
            assert np.abs(gl[:, 8:]).max() < 1e-11 * scale
            np.testing.assert_allclose(gl[:, :8], out["rj"][0].reshape(10, 8), rtol=0, atol=1e-11 * scale)
            assert abs(out["cert"][0, 1] - np.abs(gl[:, :8]).max()) <= 1e-11 * scale      # slot `dual`


def test_emulated_kernel_equals_checker_on_the_fixture_problems_and_solutions_certify_below_cold_starts(solved):
    """Slot by slot at the oracle's converged solutions (with the oracle's multipliers) and at the cold starts (none), all three lane orders,
    poisoned LDS and workspace; and the ordering: for EVERY fixture problem the oracle converges on, E at its solution is below E at its start."""
    P, X, r = solved
    ok, at_sol, at_x0 = certify_oracle_solutions(P, X, r)
    assert len(ok) >= 0.99 * len(P)
    for order in (0, 1, 2):
        es = emu_cert(P[ok], r["x"][ok], r["lam_g"][ok], r["lam_x"][ok], 10, 4, lane_order=order)
        e0 = emu_cert(P[ok], X[ok], None, None, 10, 4, lane_order=order)
        for j in range(len(ok)):
            assert_record(es["cert"][j], at_sol[j][0], at_sol[j][1], ("solution", int(ok[j]), order))
            assert_record(e0["cert"][j], at_x0[j][0], at_x0[j][1], ("start", int(ok[j]), order))
            if order == 2 and j % 16 == 0:
                assert_extras(es, j, at_sol[j][2], 10); assert_extras(e0, j, at_x0[j][2], 10)
        if order == 0:
            Es, E0 = es["cert"][:, 0], e0["cert"][:, 0]
    worst = int(np.argmax(Es / E0))
    print(f"\nE at the solution / E at the start: largest {Es[worst] / E0[worst]:.3e} (problem {int(ok[worst])}: {Es[worst]:.3e} / {E0[worst]:.3e})")
    assert (Es < E0).all(), [(int(ok[j]), Es[j], E0[j]) for j in np.flatnonzero(~(Es < E0))]
    no_pad = emu_cert(P[ok[:4]], r["x"][ok[:4]], r["lam_g"][ok[:4]], r["lam_x"][ok[:4]], 10, 4, poison=False, want=False)
    np.testing.assert_array_equal(no_pad["cert"], emu_cert(P[ok[:4]], r["x"][ok[:4]], r["lam_g"][ok[:4]], r["lam_x"][ok[:4]], 10, 4)["cert"])


@pytest.mark.parametrize("N,S", [(10, 4), (3, 2), (5, 3), (4, 5), (30, 4)])
def test_emulated_kernel_equals_checker_other_sizes_and_perturbed_points(N, S):
    """Both iterate placements (LDS for N <= 11 and S <= 4, workspace otherwise), the parameter tail of S > 4, horizons shorter and longer than a
    ten-node pass; at the oracle's solutions, at the cold starts and at perturbed interior points with partly wrong-signed multipliers."""
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(3, seed=N + S, N=N, S=S, tight=N > 10, workers=1)
    r = c_oracle.solve(P, X, N, S, 0.1, nthreads=3)
    rng = np.random.default_rng(N * S)
    Xp = r["x"] + rng.normal(size=X.shape) * 1e-3
    lg = np.where(rng.random(r["lam_g"].shape) < 0.5, r["lam_g"], rng.normal(size=r["lam_g"].shape))
    lx = r["lam_x"] + (rng.random(r["lam_x"].shape) < 0.1) * rng.normal(size=r["lam_x"].shape)
    for x, g_, x_ in ((r["x"], r["lam_g"], r["lam_x"]), (X, None, None), (Xp, lg, lx), (Xp, lg, None), (Xp, None, lx)):
        for order in (0, 1, 2):
            out = emu_cert(P, x, g_, x_, N, S, lane_order=order)
            for b in range(3):
                rec, tol, ex = checker(P[b], x[b], None if g_ is None else g_[b], None if x_ is None else x_[b], N, S)
                assert_record(out["cert"][b], rec, tol, (N, S, b, order))
                assert_extras(out, b, ex, N)


def test_gap_rules():
    p, x0 = _g6(1)
    r = c_oracle.solve(p, x0, 10, 4, 0.1, c_oracle.default_opts(tol=1e-8))
    x, lg, lx = r["x"][0], r["lam_g"][0].copy(), r["lam_x"][0].copy()
    base = emu_cert(p, x, lg, lx, 10, 4)
    cons = base["lam_g"][0]
    # NULL inputs: both gap slots 0; the consistent multipliers handed back: both gaps at rounding level
    none = emu_cert(p, x, None, None, 10, 4)["cert"][0]
    assert none[5] == 0.0 and none[6] == 0.0
    nu, sc, c, wd, H = nu_of(p, x, lg, lx, 10, 4)
    assert (np.abs(c) < wd).all()      # the solution is inside its tubes: the round trip of the inequality multipliers is exact up to rounding
    rec, tol, ex = checker(p, x, lg, lx, 10, 4)
    assert base["cert"][0, 6] <= tol["lam_ineq_gap"]
    again = emu_cert(p, x, cons, lx, 10, 4)["cert"][0]
    assert again[5] <= 1e-11 * ex["scale"] and again[6] <= tol["lam_ineq_gap"]
    # a shifted equality multiplier shows up in lam_eq_gap exactly (and nowhere else: the adjoint does not read it)
    sh = cons.copy(); sh[3 * NG + 5] += 0.375
    got = emu_cert(p, x, sh, lx, 10, 4)["cert"][0]
    assert abs(got[5] - 0.375) <= 1e-11 * ex["scale"]
    np.testing.assert_array_equal(np.delete(got, 5), np.delete(again, 5))
    # wrong-signed lam_g[36:43]: the entry counts as 0 in the certificate (nothing is re-exported for it), so the gap is its size
    for entries, predicted in ((((2 * NG + 36, -0.25),), 0.25), (((2 * NG + 36, -0.25), (4 * NG + 40, -1.5)), 1.5)):
        ws = cons.copy()
        for i, v in entries:
            ws[i] = v
        got = emu_cert(p, x, ws, lx, 10, 4)["cert"][0]
        assert abs(got[6] - predicted) <= 1e-12 * (predicted + ex["tube"] + ex["nu"].max()), (got[6], predicted)
        assert abs(got[6] - checker(p, x, ws, lx, 10, 4)[0]["lam_ineq_gap"]) <= 1e-12 * (predicted + ex["tube"] + ex["nu"].max())
    # lam_x on an unbounded variable (ddq, z = 22): nothing to map it to, the gap is its size
    ub = lx.copy(); ub[5 * NZ + 22] = 0.625
    got = emu_cert(p, x, cons, ub, 10, 4)["cert"][0]
    assert abs(got[6] - 0.625) <= tol["lam_ineq_gap"] and got[0] == again[0]
    # a point outside a tube: the violated row gets lam (wd + |c|), the gap is lam (|c| - wd) / (2 wd) (predicted from the checker's c, wd)
    xo = x.copy(); xo.reshape(10, NZ)[6, 29:32] += np.array([0.0, 0.08, 0.08])
    lam_t = np.zeros(430); lam_t.reshape(10, NG)[6, 38:43] = 2.0
    _, _, co, wo, _ = nu_of(p, xo, lam_t, None, 10, 4)
    outside = np.abs(co[6]) > wo[6]
    assert outside.any()
    predicted = (2.0 * (np.abs(co[6]) - wo[6]) / (2 * wo[6]))[outside].max()
    got = emu_cert(p, xo, lam_t, None, 10, 4)["cert"][0]
    assert predicted > 0 and abs(got[6] - predicted) <= 1e-12 * (predicted + 2.0 * ((np.abs(co[6]) + wo[6]) / wo[6]).max())
    assert got[3] > 0      # (and the point is infeasible: prim_ineq)
    # NaN and inf entries: the slot of the entry is +inf, the entry counts as 0 elsewhere
    for bad in (np.nan, np.inf, -np.inf):
        a = cons.copy(); a[7 * NG + 37] = bad
        got = emu_cert(p, x, a, lx, 10, 4)["cert"][0]
        assert got[6] == np.inf and np.isfinite(np.delete(got, 6)).all()
        a = lx.copy(); a[2 * NZ + 9] = bad
        assert emu_cert(p, x, cons, a, 10, 4)["cert"][0, 6] == np.inf
        a = cons.copy(); a[2 * NG + 4] = bad
        got = emu_cert(p, x, a, lx, 10, 4)["cert"][0]
        assert got[5] == np.inf and got[6] == again[6] and got[0] == again[0]


def test_non_finite_points_give_non_finite_records_never_a_fault():
    p, x0 = _g6(1)
    for N, S in ((10, 4), (30, 4)):
        if N == 30:
            from boundmpc_amd import workload
            P, X, _ = workload.make_batch(1, seed=1, N=N, S=S, tight=True, workers=1)
            p, x0 = P[0], X[0]
        for what in ("x", "p", "xinf", "all"):
            pp, xx = p.copy(), x0.copy()
            if what == "x":
                xx[3 * NZ + 41] = np.nan
            elif what == "xinf":
                xx[2 * NZ + 10] = np.inf
            elif what == "p":
                pp[30] = np.nan
            else:
                pp[:] = np.nan; xx[:] = np.nan
            for order in (0, 2):
                out = emu_cert(pp, xx, np.ones(N * NG), np.ones(N * NZ), N, S, lane_order=order)
                assert np.isnan(out["cert"][0, :5]).all(), (what, out["cert"][0])


def test_measured_a_converged_solve_certifies(solved):
    """The figures of profiles/kkt_certificate.txt (numpy checker on the C oracle's tol-1e-8 solutions of the fixture problems), recomputed: the
    committed file states what this tree measures.  A measurement, not a threshold on E."""
    P, X, r = solved
    ok, E, lines = measured_lines(P, X, r)
    print("\n" + "\n".join(lines))
    text = open(PROFILE).read()
    for key in ("max_E_over_tol", "max_E_over_kkt_of_the_solve"):
        have = float(re.search(rf"^{key} = (\S+)$", text, re.M).group(1))
        want = float(next(l for l in lines if l.startswith(key + " =")).split("=")[1])
        assert have == pytest.approx(want, rel=1e-3), key


# ---- C ABI and the Python argument checks ----
def test_abi_declares_exports_and_binds_the_three_entry_points():
    from boundmpc_amd import _lib, build, solver
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "boundmpc_hip.h")).read(), flags=re.S)
    assert re.search(r"int bmpc_kkt_len\(void\);", hdr)
    assert re.search(r"int bmpc_kkt_batch\(bmpc_handle \*h, int B, const double \*p, const double \*x, const double \*lam_g0, const double \*lam_x0, double \*cert,"
                     r"\s*double \*g, double \*lam_g, double \*rj, void \*hip_stream\);", hdr)
    assert re.search(r"int bmpc_kkt_batch_host\(bmpc_handle \*h, int B, const double \*p, const double \*x, const double \*lam_g0, const double \*lam_x0, double \*cert,"
                     r"\s*double \*g, double \*lam_g, double \*rj\);", hdr)
    slots = dict(re.findall(r"BMPC_KKT_(\w+) = (\d+)", hdr))
    assert [int(slots[k.upper()]) for k in solver.KKT_FIELDS] == list(range(8)) and int(slots["LEN"]) == 8 == len(FIELDS)
    assert solver.KKT_FIELDS == FIELDS and (solver.KKT_E, solver.KKT_LAM_INEQ_GAP, solver.KKT_F) == (0, 6, 7)
    assert _emu().bmpc_emu_kkt_len() == 8
    assert os.path.join(build.CSRC, "bmpc_kkt.inl") in build.SOURCES
    build.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("bmpc_kkt_len", "bmpc_kkt_batch", "bmpc_kkt_batch_host"):
        assert hasattr(lib, n) and n in _lib.SYMBOLS
    assert lib.bmpc_kkt_len() == 8
    # argument checks that need no device: a NULL handle / buffers, B < 1
    vp = ctypes.c_void_p
    lib.bmpc_kkt_batch.argtypes = [vp, ctypes.c_int] + [vp] * 9
    lib.bmpc_kkt_batch_host.argtypes = [vp, ctypes.c_int] + [vp] * 8
    assert lib.bmpc_kkt_batch(None, 1, None, None, None, None, None, None, None, None, None) == 1
    assert lib.bmpc_kkt_batch_host(None, 0, None, None, None, None, None, None, None, None) == 1


class _FakeLib:
    def __getattr__(self, n):
        raise AssertionError(f"{n}: the argument check must raise before the library is called")


def test_python_argument_checks_raise():
    from boundmpc_amd.solver import BatchedOCPSolver, NlpSolverShim
    s = BatchedOCPSolver.__new__(BatchedOCPSolver)
    s.N, s.S, s.n_w, s.n_g, s.n_p, s._lib, s._h = 10, 4, 440, 430, 505, _FakeLib(), None
    with pytest.raises(ValueError, match="shape mismatch"):
        s.certify_host(np.zeros((2, 505)), np.zeros((2, 439)))
    with pytest.raises(ValueError, match="lam_g has shape"):
        s.certify_host(np.zeros((2, 505)), np.zeros((2, 440)), lam_g=np.zeros((2, 440)))
    with pytest.raises(ValueError, match="lam_x has shape"):
        s.certify_host(np.zeros((2, 505)), np.zeros((2, 440)), lam_x=np.zeros((1, 440)))
    with pytest.raises(ValueError, match="a certificate offers"):
        s.certify_host(np.zeros((2, 505)), np.zeros((2, 440)), want=("lam_x",))
    with pytest.raises(ValueError, match="float64 tensors on the GPU"):
        import torch
        s.certify(torch.zeros((2, 505), dtype=torch.float64), torch.zeros((2, 440), dtype=torch.float64))
    shim = NlpSolverShim.__new__(NlpSolverShim)
    shim._s = s
    with pytest.raises(RuntimeError, match="previous solver"):
        shim.certificate()
