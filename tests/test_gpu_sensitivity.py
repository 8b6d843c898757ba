"""Parametric solution sensitivities on the MI355X (bmpc_service_kernel over SensBatch, boundmpc_amd/csrc/bmpc_sens.inl): dx against the numpy checker of
tests/test_sensitivity.py (its checked set, read from tests/golden/sensitivity_checked_set.npz; the same bound: 100 x the checker's own floor),
the three equations at full size, differenced real solves, and the contract cases through the device entry point, the host entry point and the
shim: zero direction, linearity, NULL multipliers, non-finite input, regularisation, argument errors, determinism, [B, D, n_p], interleaving
with solves and certificates on other streams.  `pytest -m gpu`."""
import numpy as np
import pytest

from tests.test_sensitivity import (FACTOR, H_, MU, NE, NG, NI, NZ, S_, _scale, directions, equation_residuals, floor_of, full_size_points, golden_rows,
                                    other_instantiation_point, real_solve_comparison, regularised_point, small_problems)

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


@pytest.fixture(scope="module")
def rows():
    return golden_rows()


@pytest.fixture(scope="module")
def solvers():
    from boundmpc_amd import BatchedOCPSolver
    s = {N: BatchedOCPSolver(N, S_, H_) for N in (2, 3, 10)}
    yield s
    for v in s.values():
        v.close()


def test_gpu_kernel_matches_the_checker_within_the_measured_floor(rows, solvers):
    fl = floor_of(rows)
    worst = 0.0
    for N in (2, 3):
        rs = [r for r in rows if r["N"] == N]
        st = lambda k: np.stack([r[k] for r in rs])
        o = solvers[N].sensitivity_host(st("p"), st("x"), st("dp"), lam_g=st("lam_g"), lam_x=st("lam_x"), mu=MU)
        assert (o["rec"][:, 0] == 0).all(), o["rec"]
        for i, r in enumerate(rs):
            e = np.abs(o["dx"][i] - r["dx"]).max() / _scale(r)
            print(f"  N={N} problem {r['b']} {r['name']:<11} checker twice {np.abs(r['dx'] - r['dx_central']).max() / _scale(r):.2e}  kernel {e:.2e}")
            worst = max(worst, e)
            assert o["rec"][i, 3] == np.abs(o["dx"][i]).max()
    print(f"floor = {fl:.6e}; bound = {FACTOR * fl:.6e}; gpu_discrepancy = {worst:.6e}")
    assert worst <= FACTOR * fl, (worst, fl)


def test_gpu_full_size_tangent_satisfies_the_three_equations(rows, solvers):
    fl = floor_of(rows)
    P, X, LG, LX = full_size_points()
    for b, name in ((0, "q0[1]"), (1, "dense")):
        dp = directions(P[b], X[b], 10, S_, seed=b)[name]
        o = solvers[10].sensitivity_host(P[b], X[b], dp, lam_g=LG[b], lam_x=LX[b], mu=MU, want_duals=True)
        assert o["rec"][0, 0] == 0.0
        res = equation_residuals(P[b], X[b], LG[b], LX[b], dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], 10)
        for k, (r, sc) in res.items():
            print(f"  N=10 problem {b} {name}: {k} residual {r:.3e} scale {sc:.3e} ratio {r / sc:.3e} (bound {FACTOR * fl:.3e})")
            assert r <= FACTOR * fl * sc, (b, name, k, r, sc)


@pytest.mark.parametrize("N,S", [(4, 5), (12, 4)])
def test_gpu_instantiation_without_the_lds_iterate_satisfies_the_equations(rows, N, S):
    """bmpc_service_kernel<false, SensBatch> (S > 4 or N > 11: iterate and direction in the workspace slab) on the hardware: the three equations at S = 5, the
    equality rows and the row equation at N = 12 (as the emulator test), device and host entry points bit-equal"""
    from boundmpc_amd import BatchedOCPSolver
    fl = floor_of(rows)
    p, x, lg, lx, dp = other_instantiation_point(N, S)
    s = BatchedOCPSolver(N, S, H_)
    o = s.sensitivity_host(p, x, dp, lam_g=lg, lam_x=lx, mu=MU, want_duals=True)
    dev = _np(s.sensitivity(_t(p[None]), _t(x[None]), _t(dp[None]), lam_g=_t(lg[None]), lam_x=_t(lx[None]), mu=MU, want_duals=True))
    s.close()
    for k in o:
        np.testing.assert_array_equal(dev[k].view(np.uint64), o[k].view(np.uint64), err_msg=k)
    assert o["rec"][0, 0] == 0.0
    res = equation_residuals(p, x, lg, lx, dp, o["dx"][0], o["dlam_eq"][0], o["dnu"][0], N, S=S, stationarity=N < 10)
    for k, (r, sc) in res.items():
        print(f"  N={N} S={S}: {k} residual {r:.3e} scale {sc:.3e} ratio {r / sc:.3e} (bound {FACTOR * fl:.3e})")
        assert r <= FACTOR * fl * sc, (N, S, k, r, sc)


def test_gpu_tangent_agrees_with_differenced_real_solves(solvers):
    cos, size, spread = real_solve_comparison(lambda p, x, lg, lx, dp, mu: solvers[10].sensitivity_host(p, x, dp, lam_g=lg, lam_x=lx, mu=mu)["dx"][0])
    print(f"cosine {cos:.9f}; size error {size:.3e}; spread of the finite difference: {spread:.3e}")
    assert cos >= 0.99 and size <= spread, (cos, size, spread)


def test_gpu_contract_cases(rows, solvers):
    import torch
    from boundmpc_amd import _lib
    from boundmpc_amd._lib import BoundMPCHipError
    fl = floor_of(rows)
    s = solvers[3]
    P, X, LG, LX = small_problems(3, 2)
    p, x, lg, lx = P[1], X[1], LG[1], LX[1]
    d = directions(p, x, 3, S_, seed=1)
    d1, d2 = d["q0[1]"], d["dense"]
    f = lambda dp, **kw: s.sensitivity_host(p, x, dp, lam_g=lg, lam_x=lx, mu=MU, **kw)
    # zero direction
    o = f(np.zeros_like(p), want_duals=True)
    assert (o["dx"] == 0).all() and (o["dlam_eq"] == 0).all() and (o["dnu"] == 0).all() and o["rec"][0, 0] == 0 and o["rec"][0, 2] == 0
    # linear in dp within the floor; [B, D, n_p] equals D separate calls bit for bit (device and host entry points)
    dirs = np.stack([d1, d2, 2 * d1, d1 + d2])
    many = s.sensitivity_host(p, x, dirs[None], lam_g=lg, lam_x=lx, mu=MU, want_duals=True)
    assert many["dx"].shape == (1, 4, 3 * NZ) and many["rec"].shape == (1, 4, 4) and many["dnu"].shape == (1, 4, 3 * NI) and many["dlam_eq"].shape == (1, 4, 3 * NE)
    dev = _np(s.sensitivity(_t(p[None]), _t(x[None]), _t(dirs[None]), lam_g=_t(lg[None]), lam_x=_t(lx[None]), mu=MU, want_duals=True))
    for k in many:
        np.testing.assert_array_equal(dev[k].view(np.uint64), many[k].view(np.uint64), err_msg=k)
    for i in range(4):
        one = f(dirs[i], want_duals=True)
        for k in many:
            np.testing.assert_array_equal(one[k][0].view(np.uint64), many[k][0, i].view(np.uint64), err_msg=k)
    a, b, a2, ab = many["dx"][0]
    assert np.abs(a2 - 2 * a).max() <= fl * np.abs(a2).max()
    assert np.abs(ab - (a + b)).max() <= fl * max(np.abs(a).max(), np.abs(b).max())
    # NULL multipliers equal explicit zeros bit for bit
    n0 = s.sensitivity_host(p, x, d2, mu=MU, want_duals=True)
    z0 = s.sensitivity_host(p, x, d2, lam_g=np.zeros(3 * NG), lam_x=np.zeros(3 * NZ), mu=MU, want_duals=True)
    for k in n0:
        np.testing.assert_array_equal(n0[k].view(np.uint64), z0[k].view(np.uint64), err_msg=k)
    # non-finite x, p or dp: status 3 and NaN, no fault; the neighbouring rows are untouched
    good = f(d2)["dx"][0]
    Pb, Xb, Db = np.tile(p, (4, 1)), np.tile(x, (4, 1)), np.tile(d2, (4, 1))
    Xb[1, 41] = np.nan; Pb[2, 3] = np.inf; Db[3, 5] = np.nan
    o = s.sensitivity_host(Pb, Xb, Db, lam_g=np.tile(lg, (4, 1)), lam_x=np.tile(lx, (4, 1)), mu=MU, want_duals=True)
    assert (o["rec"][1:, 0] == 3).all() and np.isnan(o["dx"][1:]).all() and np.isnan(o["dnu"][1:]).all() and np.isnan(o["dlam_eq"][1:]).all()
    assert o["rec"][0, 0] == 0
    np.testing.assert_array_equal(o["dx"][0].view(np.uint64), good.view(np.uint64))
    # a point that needs regularisation: status 1 with its delta
    pr, xr, lgr, lxr = regularised_point()
    o = s.sensitivity_host(pr, xr, d1, lam_g=lgr, lam_x=lxr, mu=1e-2)
    assert o["rec"][0, 0] == 1.0 and o["rec"][0, 1] > 0 and np.isfinite(o["dx"]).all(), o["rec"]
    # argument errors
    tp, tx, td = _t(p[None]), _t(x[None]), _t(d1[None])
    out = torch.zeros((1, 3 * NZ), dtype=torch.float64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    for args in ((0, tp, tx, td, out), (1, None, tx, td, out), (1, tp, None, td, out), (1, tp, tx, None, out), (1, tp, tx, td, None)):
        with pytest.raises(BoundMPCHipError):
            _lib.check(s._lib.bmpc_sens_batch(s._h, args[0], ptr(args[1]), ptr(args[2]), None, None, ptr(args[3]), 0.0, ptr(args[4]), None, None, None, None), "bmpc_sens_batch")
    with pytest.raises(ValueError):
        s.sensitivity(tp, tx, _t(d1[None, None, :-1]))
    # mu = None is options.tol * options.mu_min_fac (1e-8 * 0.1 = MU on a default handle)
    np.testing.assert_array_equal(s.sensitivity_host(p, x, d2, lam_g=lg, lam_x=lx)["dx"], s.sensitivity_host(p, x, d2, lam_g=lg, lam_x=lx, mu=MU)["dx"])


def test_gpu_determinism_row_and_batch_size(solvers):
    """Two launches give equal bits; a problem's tangent depends neither on its row nor on B (2 against 2049: the waves stride over the batch)."""
    import torch
    s = solvers[10]
    P, X, LG, LX = full_size_points()
    D = np.stack([directions(P[b], X[b], 10, S_, seed=b)["dense"] for b in range(2)])
    small = _np(s.sensitivity(_t(P), _t(X), _t(D), lam_g=_t(LG), lam_x=_t(LX), mu=MU, want_duals=True))
    assert 2049 > s.launch_info()["grid"]
    idx = np.arange(2049) % 2
    idx[[0, 1]] = [1, 0]
    args = [_t(a[idx]) for a in (P, X, D)]
    kw = dict(lam_g=_t(LG[idx]), lam_x=_t(LX[idx]), mu=MU, want_duals=True)
    big1 = _np(s.sensitivity(*args, **kw)); big2 = _np(s.sensitivity(*args, **kw))
    torch.cuda.synchronize()
    for k in small:
        np.testing.assert_array_equal(big1[k].view(np.uint64), big2[k].view(np.uint64), err_msg=k)
        np.testing.assert_array_equal(big1[k].view(np.uint64), small[k][idx].view(np.uint64), err_msg=k)


def test_gpu_sensitivity_between_solve_and_certify_on_other_streams_leaves_all_three_bit_equal():
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(600, seed=5)
    p, x0 = _t(P), _t(X)
    rng = np.random.default_rng(0)
    dp = _t(rng.normal(size=P.shape) * 1e-2 * np.maximum(np.abs(P), 1e-2))
    s = BatchedOCPSolver(10, 4, 0.1)
    ref = _np(s.solve_batch(p, x0, out={}))
    xs, lg, lx = _t(ref["x"]), _t(ref["lam_g"]), _t(ref["lam_x"])
    cert = _np(s.certify(p, xs, lg, lx, out={}))
    alone = _np(s.sensitivity(p, xs, dp, lam_g=lg, lam_x=lx, want_duals=True))
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for st in (s1, s2, s3):
        st.wait_stream(torch.cuda.current_stream())
    o1 = s.solve_batch(p, x0, out={}, stream=s1)
    t = s.sensitivity(p, xs, dp, lam_g=lg, lam_x=lx, want_duals=True, stream=s2)
    c = s.certify(p, xs, lg, lx, out={}, stream=s3)
    torch.cuda.synchronize()
    o1, t, c = _np(o1), _np(t), _np(c)
    for k in ref:
        np.testing.assert_array_equal(o1[k], ref[k], err_msg=k)
    for k in alone:
        np.testing.assert_array_equal(t[k].view(np.uint64), alone[k].view(np.uint64), err_msg=k)
    np.testing.assert_array_equal(c["cert"].view(np.uint64), cert["cert"].view(np.uint64))
    ok = ref["status"] == 0
    assert (alone["rec"][ok, 0] <= 1).all() and np.isfinite(alone["dx"][ok]).all()
    s.close()


def test_gpu_shim_sensitivity_of_the_last_call(solvers):
    from boundmpc_amd import NlpSolverShim
    s = solvers[10]
    P, X, LG, LX = full_size_points()
    shim = NlpSolverShim(s)
    lbx, ubx, lbg, ubg = s.bounds()
    sol = shim(x0=X[0], lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P[0])
    d = directions(P[0], X[0], 10, S_, seed=0)
    own = shim.sensitivity(d["q0[1]"])
    assert own["dx"].shape == (10 * NZ,) and own["rec"][0] == 0
    want = s.sensitivity_host(P[0], sol["x"].ravel(), d["q0[1]"], lam_g=sol["lam_g"].ravel(), lam_x=sol["lam_x"].ravel())
    np.testing.assert_array_equal(own["dx"], want["dx"][0])
    two = shim.sensitivity(np.stack([d["q0[1]"], d["dense"]]), sol={"x": X[0].reshape(-1, 1), "lam_g": LG[0], "lam_x": LX[0].reshape(-1, 1)})
    assert two["dx"].shape == (2, 10 * NZ)
    np.testing.assert_array_equal(two["dx"][0], s.sensitivity_host(P[0], X[0], d["q0[1]"], lam_g=LG[0], lam_x=LX[0])["dx"][0])
