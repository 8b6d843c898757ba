"""options.bound_margin on the MI355X against the references of tests/test_bound_margin.py (numpy checker with the margin, C oracle with the margin), on every
launch shape that reads the row table: one wave, pair, team (N = 10), the workspace-slab instantiation (N = 12) and the parameter tail (S = 5, N = 6).  Every
handle has m = 0.05; the one-wave shape also runs at the real-time mode's 2e-3.  Per shape:

  certify    the KKT kernel on the 16 crafted row points (a joint variable one micro-radian either side of its TIGHTENED limit, a jerk and phi just inside
             their untightened bounds) equals checker(bound_margin=m) within the checker's own tolerance dict;
  solve      solve_batch of the seed-0 problems (16 at N = 10, 8 otherwise) against the oracle with the margin: status equal, iterations within 2, the GPU's
             certificate of its own solution equal to checker(m) with E within the bound of profiles/bound_margin.txt, every q and dq within the tightened
             limits -- at tol 1e-8; x within 1e-7 and the multipliers within rtol = atol = 1e-6 at tol 1e-11 (why two tolerances: tests/test_bound_margin.py);
  and once   the sensitivity kernel of a margin handle at the N = 3 point with an active tightened row satisfies the three equations formed with the margin.

The condition on the inputs (the margin matters on at least 8 of the 16 problems) is asserted on the oracle's solutions first.  `pytest -m gpu`."""
import numpy as np
import pytest

from tests import test_bound_margin as bm
from tests.test_kkt_certificate import assert_record, checker

pytestmark = pytest.mark.gpu

# name -> N, S, B, set_team_waves (None: the handle's own choice), margin
SHAPES = {
    "one_wave_N10":      dict(N=10, S=4, B=16, waves=1, m=0.05),
    "one_wave_N10_2e-3": dict(N=10, S=4, B=16, waves=1, m=2e-3),
    "pair_N10":          dict(N=10, S=4, B=16, waves=2, m=0.05),
    "team_N10":          dict(N=10, S=4, B=16, waves=4, m=0.05),
    "slab_N12":          dict(N=12, S=4, B=8, waves=None, m=0.05),
    "tail_N6_S5":        dict(N=6, S=5, B=8, waves=None, m=0.05),
}


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _handle(sh, tol):
    from boundmpc_amd import BatchedOCPSolver
    s = BatchedOCPSolver(sh["N"], sh["S"], bm.H_, tol=tol, bound_margin=sh["m"])
    if sh["waves"] is not None:
        s.set_team_waves(sh["waves"])
        assert s.team_info(sh["B"])["waves"] == sh["waves"], s.team_info(sh["B"])
    return s


def _solve(s, P, X):
    import torch
    o = s.solve_batch(_t(P), _t(X), out={})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_gpu_certificate_and_solve_know_the_margin(name):
    sh = SHAPES[name]
    N, S, B, m = sh["N"], sh["S"], sh["B"], sh["m"]
    if N == 10:
        rows = bm.assert_margin_matters(m)
    P, X = bm.problems(N, S, B)
    ref = bm.oracle_solutions(m, N, S, B)[0]
    ref_x = bm.oracle_solutions(m, N, S, B, bm.TOL_X)[0]
    assert (ref["status"] == 0).all()
    p, x, lg, lx = bm.feasible_point(N, S)
    pc, pts = bm.crafted_points(N, S, m)
    s = _handle(sh, bm.TOL)
    try:
        # -- the certificate kernel on the crafted row points --
        tile = lambda a: np.tile(a, (len(pts), 1))
        got = s.certify_host(tile(pc), np.stack([q[1] for q in pts]), tile(lg), tile(lx))["cert"]
        for b, (what, xb, want) in enumerate(pts):
            rec, tol, _ = checker(pc, xb, lg, lx, N, S, bound_margin=m)
            assert_record(got[b], rec, tol, (name, what))
            assert abs(got[b, 3] - want) <= tol["prim_ineq"] + 1e-15, (name, what, got[b, 3])
        # -- the solve at the handle's default tolerance --
        o = _solve(s, P, X)
        np.testing.assert_array_equal(o["status"], ref["status"])
        assert np.abs(o["iters"] - ref["iters"]).max() <= 2, (o["iters"], ref["iters"])
        own = s.certify_host(P, o["x"], o["lam_g"], o["lam_x"])["cert"]
        bound = bm.e_bound()
        for b in range(B):
            rec, tol, _ = checker(P[b], o["x"][b], o["lam_g"][b], o["lam_x"][b], N, S, bound_margin=m)
            assert_record(own[b], rec, tol, (name, "own solution", b))
        bm.assert_within_tightened_limits(o["x"], m, N)
        dev = [float(np.abs(o[k] - ref[k]).max()) for k in ("x", "lam_g", "lam_x")]
        print(f"\n{name}: tol {bm.TOL:g}: E max {own[:, 0].max():.3e} (bound {bound:.3e}); iterations off by at most {int(np.abs(o['iters'] - ref['iters']).max())}; "
              f"against the oracle: x {dev[0]:.2e} lam_g {dev[1]:.2e} lam_x {dev[2]:.2e}")
        assert (own[:, 0] <= bound).all(), own[:, 0]
        if N == 10:      # "margin matters": the GPU's own points fail the margin-less certificate where the oracle's do
            E0g = np.array([checker(P[b], o["x"][b], o["lam_g"][b], o["lam_x"][b], N, S)[0]["E"] for b in rows])
            assert (E0g >= 1e-5 / 2).all(), E0g
    finally:
        s.close()
    # -- x and the multipliers, both sides solved to 1e-11 --
    s = _handle(sh, bm.TOL_X)
    try:
        bm.assert_same_point(_solve(s, P, X), ref_x, name)
    finally:
        s.close()


def test_gpu_tangent_on_a_margin_handle_satisfies_the_three_equations_with_the_margin():
    from boundmpc_amd import BatchedOCPSolver
    from tests import test_sensitivity as ts
    m, N = 0.05, 3
    p, x, lg, lx, dp, joint = bm.sensitivity_point(m, N)
    bound = ts.FACTOR * ts.floor_of(ts.golden_rows())      # (the committed checked set: test_golden_checked_set_is_what_the_checker_computes)
    s = BatchedOCPSolver(N, ts.S_, ts.H_, bound_margin=m)
    try:
        o = s.sensitivity_host(p, x, dp, lam_g=lg, lam_x=lx, mu=ts.MU, want_duals=True)
    finally:
        s.close()
    assert o["rec"][0, 0] == 0.0
    worst = {}
    for what, mm in (("with", m), ("without", 0.0)):
        res = ts.equation_residuals(p, x, lg, lx, dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], N, bound_margin=mm)
        worst[what] = max(r / sc for r, sc in res.values())
        print(f"\nresiduals formed {what} the margin: " + ", ".join(f"{k} {r / sc:.3e}" for k, (r, sc) in res.items()) + f" (bound {bound:.3e})")
    assert worst["with"] <= bound and worst["without"] > bound, worst
