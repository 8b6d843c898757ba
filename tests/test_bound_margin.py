"""options.bound_margin (include/boundmpc_hip.h: joint position / velocity limits tightened by m inside the solver) against references that do not
share the kernel text.  The margin enters the wave program in one line (boundmpc_amd/csrc/bmpc_wave.inl wave_init_tables: the row table's limits of rows
IQU..IPHI0); the solve, the restoration phase, bmpc_kkt_batch and bmpc_sens_batch inherit it from that table.  Here, without a GPU:

  rows         the emulated KKT kernel at crafted points one micro-radian either side of a tightened limit, against the numpy checker with the margin
               (oracle/nlp.internal_ineq(bound_margin=m): rows 16:44 only -- a jerk and phi just inside their UNtightened bounds ride along);
  solve        the lane emulator against the C oracle with the same margin (oracle/bmpc_oracle.c eval) on 16 benchmark problems, the numpy certificate
               with the margin, the tightened limits themselves;
  minimiser    the emulator against scipy SLSQP with tightened lbx / ubx (fixture g15, tests/golden/make_g15.py);
  sensitivity  the emulated tangent at a point with an active tightened row satisfies the three equations formed WITH the margin and not without.

CONDITION ON THE INPUTS (asserted on the oracle's solutions before anything else is looked at): on at least 8 of the 16 problems the margin-less
certificate of the margin solution is >= 1e-5, three decades above the certificate with the margin -- the margin matters there, and a reference without
it would say so.  tests/test_gpu_bound_margin.py holds the device to the same references on every launch shape.

TWO SOLVER TOLERANCES.  Status, iteration counts (within 2), the certificate and the limits are compared on solves at tol = 1e-8, the handle's default.
Two codes that both stop at a KKT error of 1e-8 need not agree in x to 1e-7: the joint jerks carry the curvature 2 w_jerk = 2e-4 (weights[13] = 1e-4) and
nothing else, so a stationarity residual r leaves them free by r / 2e-4 -- at MARGIN 0 the oracle and the emulator differ by 7.8e-6 in a jerk on these
problems, one iteration apart.  x within 1e-7 therefore needs r <= 2e-11: x and the multipliers are compared on solves at tol = 1e-11 (status 0 on both
sides asserted; iteration counts are not compared there -- that close to the rounding floor of the residuals they wander by more than 2).

BOUND ON E (profiles/bound_margin.txt, by the rule of profiles/kkt_certificate.txt): 10 x the largest E / tol the ORACLE's margin solutions reach under
the numpy checker; test_measured_profile recomputes the committed figure."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import c_oracle, nlp
from tests.emu import emu
from tests.test_kkt_certificate import NG, NI, NZ, assert_record, checker, emu_cert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "bound_margin.txt")
G15 = os.path.join(ROOT, "tests", "golden", "g15_scipy_margin.npz")
H_, TOL, TOL_X = 0.1, 1e-8, 1e-11
MARGINS = (2e-3, 0.05)            # the real-time mode's and a large one
ROW_MARGINS = (0.0, 2e-3, 0.05, 0.5)
OTHER_SIZES = ((12, 4), (6, 5))
LIM = np.concatenate([nlp.Q_LIM, nlp.DQ_LIM])      # of the stage variables 8:22


# ---- rows -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def feasible_point(N, S):
    """(p, x, lam_g, lam_x): an oracle solution at margin 0.5 -- strictly inside every row at every margin of ROW_MARGINS -- with its multipliers"""
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(1, seed=0, N=N, S=S, workers=1)
    r = c_oracle.solve(P, X, N, S, H_, c_oracle.opts_for(N, tol=TOL, bound_margin=0.5))
    assert r["status"][0] == 0
    out = P[0], r["x"][0], r["lam_g"][0], r["lam_x"][0]
    for a in out:
        a.setflags(write=False)
    return out


def crafted_points(N, S, m):
    """(p, 16 points [(name, x, expected prim_ineq)]): one joint variable of one stage at +-(lim - m) +- 1e-6 -- q and dq, upper and lower, first and last
    stage, outside and inside -- each with a jerk at 35 - m / 2; and phi_max of p at the largest phi of the point + m / 2 (moving phi itself would move the
    tubes), so that phi = phi_max - m / 2 there: a margin on the jerk or phi rows would call either violated."""
    p, x, _, _ = feasible_point(N, S)
    p = p.copy()
    p[nlp.p_layout(S)["phi_max"][0]] = x.reshape(N, NZ)[:, 41].max() + m / 2
    pts = []
    for n, (var, sign, stage) in enumerate((v, s, k) for v in (0, 1) for s in (1, -1) for k in (0, N - 1)):
        for side in (1, -1):      # outside, inside
            j = (3 * n + 1) % 7
            z = x.reshape(N, NZ).copy()
            z[stage, 8 + 7 * var + j] = sign * ((LIM[7 * var + j] - m) + side * 1e-6)
            z[stage, (n + 2) % 8] = -sign * (nlp.U_LIM - m / 2)
            pts.append((f"{'dq' if var else 'q'}{j} {'upper' if sign > 0 else 'lower'} stage {stage} {'outside' if side > 0 else 'inside'}", z.ravel(), 1e-6 if side > 0 else 0.0))
    return p, pts


@pytest.mark.parametrize("m", ROW_MARGINS)
@pytest.mark.parametrize("N,S", [(3, 2), (10, 4)])
def test_emulated_kkt_kernel_knows_the_margin_on_the_joint_rows_only(N, S, m):
    p, x, lg, lx = feasible_point(N, S)
    H = nlp.internal_ineq(x, p, N, S, bound_margin=0.5)
    assert H.max() < 0      # the condition on the base point
    p, pts = crafted_points(N, S, m)
    out = emu_cert(np.tile(p, (len(pts), 1)), np.stack([q[1] for q in pts]), np.tile(lg, (len(pts), 1)), np.tile(lx, (len(pts), 1)), N, S, bound_margin=m)
    for b, (name, xb, want) in enumerate(pts):
        rec, tol, _ = checker(p, xb, lg, lx, N, S, bound_margin=m)
        assert abs(rec["prim_ineq"] - want) <= 1e-13 + 1e-12 * want, (name, rec["prim_ineq"])      # (the numpy reference itself: 1e-6 outside, 0 inside)
        assert_record(out["cert"][b], rec, tol, (N, S, m, name))
        assert abs(out["cert"][b, 3] - want) <= tol["prim_ineq"] + 1e-15, (name, out["cert"][b, 3])


# ---- solve -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def problems(N=10, S=4, B=16):
    from boundmpc_amd import workload
    P, X, _ = workload.make_batch(B, seed=0, N=N, S=S, workers=1)
    P.setflags(write=False); X.setflags(write=False)
    return P, X


@functools.lru_cache(maxsize=None)
def oracle_solutions(m, N=10, S=4, B=16, tol=TOL):
    """the C oracle with the margin on the seed-0 problems; per problem the numpy certificate E with the margin and without -> (result, E, E margin-less)"""
    P, X = problems(N, S, B)
    r = c_oracle.solve(P, X, N, S, H_, c_oracle.opts_for(N, tol=tol, bound_margin=m), nthreads=8)
    for a in r.values():
        a.setflags(write=False)
    E = np.array([checker(P[b], r["x"][b], r["lam_g"][b], r["lam_x"][b], N, S, bound_margin=m)[0]["E"] for b in range(B)])
    E0 = np.array([checker(P[b], r["x"][b], r["lam_g"][b], r["lam_x"][b], N, S)[0]["E"] for b in range(B)])
    return r, E, E0


def assert_margin_matters(m):
    """the condition on the inputs; returns the rows on which the margin matters"""
    r, E, E0 = oracle_solutions(m)
    assert (r["status"] == 0).all(), r["status"]
    rows = np.flatnonzero(E0 >= 1e-5)
    assert len(rows) >= 8, (m, E0)
    return rows


def measured_lines():
    lines = [f"tol = {TOL:g}"]
    worst = 0.0
    for m in MARGINS:
        r, E, E0 = oracle_solutions(m)
        worst = max(worst, E.max() / TOL)
        lines += [f"m = {m:g}: problems = 16 (converged: {int((r['status'] == 0).sum())}) max_E = {E.max():.6e} margin_matters_on = {int((E0 >= 1e-5).sum())}",
                  f"m = {m:g}: margin-less E per problem = " + " ".join(f"{e:.1e}" for e in E0)]
    for N, S in OTHER_SIZES:      # the other problem sets of tests/test_gpu_bound_margin.py
        r, E, E0 = oracle_solutions(0.05, N, S, 8)
        worst = max(worst, E[r["status"] == 0].max() / TOL)
        lines.append(f"m = 0.05, N = {N}, S = {S}: problems = 8 (converged: {int((r['status'] == 0).sum())}) max_E = {E[r['status'] == 0].max():.6e} margin_matters_on = {int((E0 >= 1e-5).sum())}")
    return lines + [f"max_E_over_tol = {worst:.6f}"]


def e_bound():
    """10 x the largest E / tol of the oracle's margin solutions under the numpy checker, as committed in profiles/bound_margin.txt"""
    return 10.0 * float(re.search(r"^max_E_over_tol = (\S+)$", open(PROFILE).read(), re.M).group(1)) * TOL


def assert_within_tightened_limits(x, m, N=10):
    """every q and dq of every stage (stage variables: stage >= 1 of the horizon; the measured state is a parameter) within lim - m + 1e-8"""
    z = np.abs(np.asarray(x).reshape(-1, N, NZ)[:, :, 8:22])
    assert (z <= LIM - m + 1e-8).all(), float((z - (LIM - m)).max())


def assert_same_point(got, ref, what):
    """two solves at TOL_X: status 0 on both sides, x within 1e-7, multipliers within rtol = atol = 1e-6 (test_gpu_parity.test_tick0_against_oracle_and_numpy_kkt)"""
    assert (ref["status"] == 0).all() and (np.asarray(got["status"]) == 0).all(), (what, ref["status"], got["status"])
    d = [float(np.abs(np.asarray(got[k]) - ref[k]).max()) for k in ("x", "lam_g", "lam_x")]
    print(f"\n{what}: against the oracle at tol {TOL_X:g}: x {d[0]:.2e} lam_g {d[1]:.2e} lam_x {d[2]:.2e}")
    np.testing.assert_allclose(got["x"], ref["x"], rtol=0, atol=1e-7)
    np.testing.assert_allclose(got["lam_g"], ref["lam_g"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(got["lam_x"], ref["lam_x"], rtol=1e-6, atol=1e-6)


def test_measured_profile():
    """profiles/bound_margin.txt states what this tree measures (the bound of the GPU module rests on it).  A measurement, not a threshold on E."""
    lines = measured_lines()
    print("\n" + "\n".join(lines))
    have = float(re.search(r"^max_E_over_tol = (\S+)$", open(PROFILE).read(), re.M).group(1))
    assert have == pytest.approx(float(lines[-1].split("=")[1]), rel=1e-3)


@pytest.mark.parametrize("m", MARGINS)
def test_emulated_solve_equals_the_oracle_with_the_margin_and_certifies(m):
    rows = assert_margin_matters(m)
    P, X = problems()
    r, E, E0 = oracle_solutions(m)
    e = emu.solve(P, X, 10, 4, H_, opts=emu.default_opts(tol=TOL, bound_margin=m), nthreads=8)
    np.testing.assert_array_equal(e["status"], r["status"])
    assert np.abs(e["iters"] - r["iters"]).max() <= 2, (e["iters"], r["iters"])
    assert_same_point(emu.solve(P, X, 10, 4, H_, opts=emu.default_opts(tol=TOL_X, bound_margin=m), nthreads=8), oracle_solutions(m, tol=TOL_X)[0], m)
    bound = e_bound()
    Ee = np.array([checker(P[b], e["x"][b], e["lam_g"][b], e["lam_x"][b], 10, 4, bound_margin=m)[0]["E"] for b in range(16)])
    Ee0 = np.array([checker(P[b], e["x"][b], e["lam_g"][b], e["lam_x"][b], 10, 4)[0]["E"] for b in range(16)])
    print(f"\nm = {m:g}: E with the margin max {Ee.max():.3e} (bound {bound:.3e}); without, on the {len(rows)} rows where it matters: min {Ee0[rows].min():.3e}")
    assert (Ee <= bound).all(), Ee
    assert (Ee0[rows] >= 1e-5 / 2).all(), Ee0[rows]      # "margin matters": the emulator's own points fail the margin-less certificate there too
    assert_within_tightened_limits(e["x"], m)
    # and the margin moves the solution: against the margin-0 solve, far more than the 1e-7 above
    r0 = oracle_solutions(0.0)[0]
    assert np.abs(e["x"] - r0["x"]).max(axis=1)[rows].min() > 1e-4


def test_emulated_solve_lands_on_the_independent_minimiser_g15():
    """scipy SLSQP with lbx / ubx of q and dq tightened by m = 0.05 (fixture g15; two problems whose margin-less certificate is >= 1e-3): the same
    minimiser, joint-angle RMS < 1e-6 as for g8 (tests/test_oracle_golden.test_scipy_independent_solution)."""
    d = np.load(G15)
    m = float(d["m"])
    e = emu.solve(d["p"], d["x0"], 10, 4, H_, opts=emu.default_opts(tol=TOL, bound_margin=m), nthreads=2)
    assert (e["status"] == 0).all()
    for b in range(len(d["p"])):
        E0 = checker(d["p"][b], e["x"][b], e["lam_g"][b], e["lam_x"][b], 10, 4)[0]["E"]
        assert E0 >= 1e-3, E0      # the condition on the fixture's problems
        z, zs = e["x"][b].reshape(10, NZ), d["x"][b].reshape(10, NZ)
        rms_q = np.sqrt(np.mean((z[:, 8:15] - zs[:, 8:15]) ** 2))
        print(f"\ng15 problem {int(d['idx'][b])}: joint-angle RMS {rms_q:.3e}, f {e['f'][b]:.10g} / SLSQP {float(d['f'][b]):.10g}")
        assert rms_q < 1e-6, rms_q
        assert abs(e["f"][b] - float(d["f"][b])) < 1e-9 * abs(float(d["f"][b]))
        g = nlp.nlp_eval(d["x"][b], d["p"][b], 10, 4, H_)[1].reshape(10, NG)      # (the fixture itself: feasible, and inside the tightened bounds)
        assert np.abs(g[:, :36]).max() < 1e-12 and g[:, 36:].max() < 1e-12
        assert_within_tightened_limits(zs.ravel(), m)


# ---- sensitivity ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sensitivity_point(m=0.05, N=3):
    """One N = 3 problem with an active TIGHTENED joint row (active_rows with the margin, a row of 16:44) at its solution: the first such tick of a closed
    loop of the oracle with the margin from rest (stream functions on the CPU build; the plant reaches a velocity limit after some twenty ticks), and a
    direction of p that moves the measured joint state -> (p, x, lam_g, lam_x, dp, the active joint rows)."""
    from boundmpc_amd import stream as bstream, workload
    from tests import test_sensitivity as ts
    from tests.closed_loop import cpu_mirror_loop
    q0 = workload.random_q0(3, seed=7)[0]
    mpc, p0fk = workload.make_mpc(q0, N=N)
    rec = bstream.robot_record(q0, np.zeros(7), np.zeros(7), p0fk, np.zeros(6), np.array([mpc.phi_max[0], 0, 0]), np.zeros(7))
    kw = dict(tol=ts.TOL, bound_margin=m)
    for c in cpu_mirror_loop(mpc, rec, 40, N=N, first_cap=200, cap=200, opts_kw=kw):
        r = c_oracle.solve(c["p"], c["x0"], N, ts.S_, H_, c_oracle.default_opts(**kw))
        if r["status"][0] != 0:
            continue
        act = ts.active_rows(c["p"], r["x"][0], r["lam_g"][0], r["lam_x"][0], N, bound_margin=m)
        joint = tuple(int(a) for a in act if 16 <= a % NI < 44)
        if joint:
            lay = nlp.p_layout(ts.S_)
            dp = np.zeros(c["p"].size)
            dp[lay["dq0"][0]:lay["dq0"][0] + 7] = 1.0; dp[lay["q0"][0]:lay["q0"][0] + 7] = 0.5
            return c["p"].copy(), r["x"][0], r["lam_g"][0], r["lam_x"][0], dp, joint
    raise AssertionError("no tick of the N = 3 closed loop has an active tightened joint row")


def test_emulated_tangent_satisfies_the_three_equations_with_the_margin_and_not_without():
    from tests import test_sensitivity as ts
    m, N = 0.05, 3
    p, x, lg, lx, dp, joint = sensitivity_point(m, N)
    assert not any(a in joint for a in ts.active_rows(p, x, lg, lx, N)), "the row is active only under the margin"
    bound = ts.FACTOR * ts.floor_of(ts.golden_rows())      # (the committed checked set: test_golden_checked_set_is_what_the_checker_computes)
    o = ts.emu_sens(p, x, dp, lg, lx, N, opts=emu.default_opts(bound_margin=m))
    assert o["rec"][0, 0] == 0.0
    worst = {}
    for name, mm in (("with", m), ("without", 0.0)):
        res = ts.equation_residuals(p, x, lg, lx, dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], N, bound_margin=mm)
        worst[name] = max(r / sc for r, sc in res.values())
        print(f"\nresiduals formed {name} the margin: " + ", ".join(f"{k} {r / sc:.3e}" for k, (r, sc) in res.items()) + f" (bound {bound:.3e})")
    assert worst["with"] <= bound, worst
    assert worst["without"] > bound, worst
