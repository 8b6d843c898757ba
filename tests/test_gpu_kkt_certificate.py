"""KKT certificate of any primal-dual point on the MI355X (bmpc_service_kernel over KktBatch, boundmpc_amd/csrc/bmpc_kkt.inl): the record against the numpy checker of
tests/test_kkt_certificate.py (same inputs, same tolerances) through the device entry point, the host entry point and the shim; determinism;
interleaving with solves on other streams; the GPU solve's own outputs of configs[1] at full size; stale rows.  `pytest -m gpu`."""
import os
import re

import numpy as np
import pytest

from tests.test_kkt_certificate import FIELDS, NG, NZ, PROFILE, assert_extras, assert_record, checker, fixture_problems

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _np(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def _cases(P, X, r, seed):
    """(x, lam_g, lam_x): the solutions with their multipliers, the cold starts with none, perturbed points with partly wrong-signed multipliers"""
    rng = np.random.default_rng(seed)
    Xp = r["x"] + rng.normal(size=X.shape) * 1e-3
    lg = np.where(rng.random(r["lam_g"].shape) < 0.5, r["lam_g"], rng.normal(size=r["lam_g"].shape))
    lx = r["lam_x"] + (rng.random(r["lam_x"].shape) < 0.1) * rng.normal(size=r["lam_x"].shape)
    return ((r["x"], r["lam_g"], r["lam_x"]), (X, None, None), (Xp, lg, lx), (Xp, lg, None), (Xp, None, lx))


def _check(out, P, x, lg, lx, N, S, rows, what):
    for b in rows:
        rec, tol, ex = checker(P[b], x[b], None if lg is None else lg[b], None if lx is None else lx[b], N, S)
        assert_record(out["cert"][b], rec, tol, (what, N, S, int(b)))
        for i, k in enumerate(FIELDS):
            assert out[k][b] == out["cert"][b, i] or (np.isnan(out[k][b]) and np.isnan(out["cert"][b, i]))
        if "g" in out:
            assert_extras(out, b, ex, N)


@pytest.mark.parametrize("N,S,B", [(10, 4, None), (30, 4, 6), (4, 5, 6)])
def test_gpu_record_equals_checker_device_host_and_shim(N, S, B):
    """Both kernel instantiations (iterate in LDS: N = 10 / S = 4; iterate in the workspace: N = 30, and S = 5), on the fixture problems of the
    CPU test (N = 10) and on oracle-solved synthetic problems (other sizes), through certify, certify_host and NlpSolverShim.certificate."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, NlpSolverShim, workload
    from oracle import c_oracle
    if B is None:
        P, X = fixture_problems()
        r = c_oracle.solve(P, X, N, S, 0.1, c_oracle.default_opts(tol=1e-8), nthreads=8)
        rows = np.arange(0, len(P), 7)
    else:
        P, X, _ = workload.make_batch(B, seed=N + S, N=N, S=S, tight=N > 10, workers=1)
        r = c_oracle.solve(P, X, N, S, 0.1, nthreads=8)
        rows = np.arange(B)
    s = BatchedOCPSolver(N, S, 0.1)
    for x, lg, lx in _cases(P, X, r, N * S):
        dev = s.certify(_t(P), _t(x), _t(lg), _t(lx), want=("g", "lam_g", "rj"))
        torch.cuda.synchronize()
        dev = _np(dev)
        _check(dev, P, x, lg, lx, N, S, rows, "device")
        host = s.certify_host(P, x, lg, lx, want=("g", "lam_g", "rj"))
        for k in dev:      # the host entry point runs the same kernel on staged copies
            np.testing.assert_array_equal(host[k], dev[k], err_msg=k)
        lean = _np(s.certify(_t(P), _t(x), _t(lg), _t(lx)))
        np.testing.assert_array_equal(lean["cert"], dev["cert"])
        assert "g" not in lean
    # the shim: a CasADi-style result for the p of the last call; default = the last solution
    shim = NlpSolverShim(s)
    lbx, ubx, lbg, ubg = s.bounds()
    for b in rows[:2]:
        sol = shim(x0=X[b], lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P[b])
        own = shim.certificate()
        rec, tol, _ = checker(P[b], sol["x"].ravel(), sol["lam_g"].ravel(), sol["lam_x"].ravel(), N, S)
        assert_record([own[k] for k in FIELDS], rec, tol, ("shim", int(b)))
        other = shim.certificate({"x": r["x"][b].reshape(-1, 1), "lam_g": r["lam_g"][b], "lam_x": r["lam_x"][b].reshape(-1, 1)})
        rec, tol, _ = checker(P[b], r["x"][b], r["lam_g"][b], r["lam_x"][b], N, S)
        assert_record([other[k] for k in FIELDS], rec, tol, ("shim, the oracle's answer", int(b)))
        start = shim.certificate({"x": X[b]})
        assert start["lam_eq_gap"] == 0.0 and start["lam_ineq_gap"] == 0.0 and start["E"] > own["E"]
    shim.close(); s.close()


def test_gpu_argument_checks_and_hostile_points():
    import torch
    from boundmpc_amd import BatchedOCPSolver, _lib
    from boundmpc_amd._lib import BoundMPCHipError
    P, X = fixture_problems()
    P, X = P[:4].copy(), X[:4].copy()
    s = BatchedOCPSolver(10, 4, 0.1)
    with pytest.raises(ValueError):
        s.certify(_t(P), _t(X), lam_g=_t(np.zeros((4, 440))))
    with pytest.raises(ValueError):
        s.certify(_t(P), _t(X), want=("lam_x",))
    with pytest.raises(ValueError):
        s.certify(_t(P), _t(X), out={"cert": torch.zeros((4, 7), dtype=torch.float64, device="cuda")})
    with pytest.raises(BoundMPCHipError):      # B < 1
        _lib.check(s._lib.bmpc_kkt_batch(s._h, 0, None, None, None, None, None, None, None, None, None), "bmpc_kkt_batch")
    with pytest.raises(BoundMPCHipError):      # NULL cert
        _lib.check(s._lib.bmpc_kkt_batch(s._h, 4, _t(P).data_ptr(), _t(X).data_ptr(), None, None, None, None, None, None, None), "bmpc_kkt_batch")
    assert s.certify(_t(P), _t(X), lam_g=0, lam_x=0)["lam_ineq_gap"].cpu().numpy().max() == 0.0
    # non-finite x / p: a non-finite record, never a fault; the neighbouring rows are untouched
    good = s.certify_host(P, X)["cert"].copy()
    Xb, Pb = X.copy(), P.copy()
    Xb[1, 3 * NZ + 41] = np.nan; Xb[2, :] = np.inf; Pb[3, :] = np.nan
    got = s.certify_host(Pb, Xb, np.ones((4, 430)), np.ones((4, 440)))["cert"]
    assert np.isnan(got[1:, :5]).all() and np.isfinite(got[0]).all()
    np.testing.assert_array_equal(s.certify_host(P, X)["cert"], good)
    s.close()


def test_gpu_determinism_row_and_batch_size():
    """Two launches give equal bits; a problem's record depends neither on its row nor on B (3 against 2049: the waves stride over the batch)."""
    import torch
    from boundmpc_amd import BatchedOCPSolver
    from oracle import c_oracle
    P, X = fixture_problems()
    P, X = P[:3], X[:3]
    r = c_oracle.solve(P, X, 10, 4, 0.1)
    s = BatchedOCPSolver(10, 4, 0.1)
    grid = s.launch_info()["grid"]
    assert 2049 > grid      # the large batch strides the resident waves
    small = _np(s.certify(_t(P), _t(r["x"]), _t(r["lam_g"]), _t(r["lam_x"]), want=("g", "lam_g", "rj")))
    idx = np.arange(2049) % 3
    idx[[0, 1, 2]] = [2, 0, 1]      # (and not in the order of the small batch)
    args = [_t(a[idx]) for a in (P, r["x"], r["lam_g"], r["lam_x"])]
    big1 = _np(s.certify(*args, want=("g", "lam_g", "rj")))
    big2 = _np(s.certify(*args, want=("g", "lam_g", "rj")))
    torch.cuda.synchronize()
    for k in ("cert", "g", "lam_g", "rj"):
        np.testing.assert_array_equal(big1[k].view(np.uint64), big2[k].view(np.uint64), err_msg=k)
        np.testing.assert_array_equal(big1[k].view(np.uint64), small[k][idx].view(np.uint64), err_msg=k)
    s.close()


def test_gpu_certify_between_solves_on_other_streams_leaves_them_bit_equal():
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(600, seed=5)
    p, x0 = _t(P), _t(X)
    s = BatchedOCPSolver(10, 4, 0.1)
    ref1, ref2 = _np(s.solve_batch(p, x0, out={})), _np(s.solve_batch(p[:300], x0[:300], out={}))
    xs, lg, lx = _t(ref1["x"]), _t(ref1["lam_g"]), _t(ref1["lam_x"])
    alone = _np(s.certify(p, xs, lg, lx, out={}))
    torch.cuda.synchronize()
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    for st in (s1, s2, s3):
        st.wait_stream(torch.cuda.current_stream())
    o1 = s.solve_batch(p, x0, out={}, stream=s1)
    c = s.certify(p, xs, lg, lx, out={}, stream=s2)
    o2 = s.solve_batch(p[:300], x0[:300], out={}, stream=s3)
    torch.cuda.synchronize()
    o1, o2, c = _np(o1), _np(o2), _np(c)
    for k in ref1:
        np.testing.assert_array_equal(o1[k], ref1[k], err_msg=k)
        np.testing.assert_array_equal(o2[k], ref2[k], err_msg=k)
    np.testing.assert_array_equal(c["cert"].view(np.uint64), alone["cert"].view(np.uint64))
    s.close()


@pytest.fixture(scope="module")
def c1():
    """configs[1] (B = 1024, seed 0) solved on the GPU, certified with its own outputs."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(1024, seed=0)
    s = BatchedOCPSolver(10, 4, 0.1)
    o = s.solve_batch(_t(P), _t(X))
    c = s.certify(_t(P), o["x"], o["lam_g"], o["lam_x"])
    torch.cuda.synchronize()
    yield s, P, X, _np(o), _np(c)
    s.close()


def test_gpu_configs1_solutions_certify(c1):
    """Every status-0 problem of the full batch: E <= 10 x the oracle-measured maximum of profiles/kkt_certificate.txt (the factor covers GPU
    iterates that stop an iteration or two away from the oracle's); lam_ineq_gap at rounding level: a solve's own multipliers come back from the
    map and its inverse a few ulp of the multiplier apart (the point is inside its tubes), bounded here by 1e-12 (1 + 4 max |lam|).  No problem is excluded."""
    s, P, X, o, c = c1
    text = open(PROFILE).read()
    bound = 10.0 * float(re.search(r"^max_E_over_tol = (\S+)$", text, re.M).group(1)) * float(re.search(r"^tol = (\S+)$", text, re.M).group(1))
    ok = o["status"] == 0
    assert ok.mean() > 0.99
    E, gap = c["E"][ok], c["lam_ineq_gap"][ok]
    print(f"\nconfigs[1]: {int(ok.sum())} converged; E max {E.max():.3e} median {np.median(E):.3e} (bound {bound:.3e}); E / kkt max {(E / o['kkt'][ok]).max():.3f}; "
          f"lam_ineq_gap max {gap.max():.3e}; lam_eq_gap max {c['lam_eq_gap'][ok].max():.3e}")
    assert np.isfinite(E).all() and (E <= bound).all(), (int((E > bound).sum()), E.max())
    lam_max = np.maximum(np.abs(o["lam_g"][ok]).max(axis=1), np.abs(o["lam_x"][ok]).max(axis=1))
    assert (gap <= 1e-12 * (1.0 + 4.0 * lam_max)).all(), (gap / (1.0 + lam_max)).max()
    for b in np.flatnonzero(ok)[::97]:      # and the records themselves against the checker
        rec, tol, _ = checker(P[b], o["x"][b], o["lam_g"][b], o["lam_x"][b], 10, 4)
        assert_record(c["cert"][b], rec, tol, ("configs[1]", int(b)))


def test_gpu_stale_rows_certify_worse_than_every_matched_row(c1):
    """Problem b's outputs against problem b + 1's p (what a skipped launch leaves behind): E above EVERY E of the matched rows.  An ordering."""
    s, P, X, o, c = c1
    ok = o["status"] == 0
    stale = _np(s.certify(_t(np.roll(P, -1, axis=0)), _t(o["x"]), _t(o["lam_g"]), _t(o["lam_x"]), out={}))
    both = ok      # (the stale point of row b is a converged solve's output; its p is row b + 1's)
    print(f"\nstale rows: E min {stale['E'][both].min():.3e}; matched rows: E max {c['E'][ok].max():.3e}")
    assert stale["E"][both].min() > c["E"][ok].max()
