"""Primal-dual warm start on the MI355X: the conversion kernel (bmpc_service_kernel over DualBatch, boundmpc_amd/csrc/bmpc_dual.inl) against the numpy checker
of tests/test_dual_warm_start.py, warm solves from multipliers against the oracle on every launch shape, the drop-in closed loop with the
reference's lam_g0 / lam_x0 hand-over restored, the unchanged default path, hostile input and cross-stream ordering.  `pytest -m gpu`."""
import os

import numpy as np
import pytest

from tests.test_dual_warm_start import assert_state_close, checker, round_trip_bound

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
NI = 57


def _rms_q(a, b, N=10):
    return float(np.sqrt(np.mean((a - b).reshape(-1, N, 44)[:, :, 8:15] ** 2)))


def _t(a):
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


@pytest.fixture(scope="module")
def c1():
    """configs[1] (B = 1024, seed 0) solved cold on the GPU, with the converged dual state of a warm-path solve."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(1024, seed=0)
    s = BatchedOCPSolver(10, 4, 0.1)
    p, x0 = _t(P), _t(X)
    o = s.solve_batch(p, x0)
    st = s.new_state(1024)
    ow = s.solve_batch(p, x0, out={}, state=st)      # (zeroed state: the cold start of the warm path, leaves the converged dual state)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in o.items()}
    rw = {k: v.cpu().numpy() for k, v in ow.items()}
    yield s, P, X, r, rw, st.cpu().numpy()
    s.close()


def test_conversion_kernel_equals_checker_configs1(c1):
    s, P, X, r, _, _ = c1
    for x in (X, r["x"]):
        st = s.state_from_multipliers(_t(P), _t(x), _t(r["lam_g"]), _t(r["lam_x"])).cpu().numpy()
        want, scale = checker(P, x, r["lam_g"], r["lam_x"], 10, 4)
        assert_state_close(st, want, scale, 10)


def test_conversion_round_trip_against_the_gpus_own_state(c1):
    _, P, _, _, rw, st = c1
    ok = rw["status"] == 0
    chk, _ = checker(P[ok], rw["x"][ok], rw["lam_g"][ok], rw["lam_x"][ok], 10, 4)
    nu = st[ok, :10 * NI]
    err = np.abs(chk[:, :10 * NI] - nu)
    assert (err <= round_trip_bound(P[ok], rw["x"][ok], nu, 10, 4) + 1e-12).all() and err.max() < 1e-5


@pytest.mark.parametrize("N,S,B", [(3, 2, 64), (11, 4, 64), (20, 5, 32), (40, 6, 16), (30, 4, 256)])
def test_conversion_kernel_other_handles(N, S, B):
    """LDS iterate (N <= 11, S <= 4) and workspace iterate; (30, 4, 256): a configs[3] sample (tight tubes, seed 2)."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(B, seed=2 if N == 30 else N, N=N, S=S, tight=N >= 20)
    s = BatchedOCPSolver(N, S, 0.1)
    o = s.solve_batch(_t(P), _t(X))
    torch.cuda.synchronize()
    lg, lx, x = o["lam_g"].cpu().numpy(), o["lam_x"].cpu().numpy(), o["x"].cpu().numpy()
    rng = np.random.default_rng(N)
    lg2 = np.where(rng.random(lg.shape) < 0.3, -lg, lg)
    for xx, g in ((x, lg), (X, lg2)):
        st = s.state_from_multipliers(_t(P), _t(xx), _t(g), _t(lx), mu0=0.05).cpu().numpy()
        want, scale = checker(P, xx, g, lx, N, S, mu0=0.05)
        assert_state_close(st, want, scale, N)
    s.close()


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_warm_solve_from_multipliers_matches_oracle(c1, waves):
    """solve_batch(p, x0, lam_g0=, lam_x0=) against the checker's state fed to the oracle, on the one-wave, pair and team kernels."""
    import torch
    from boundmpc_amd import BatchedOCPSolver
    from oracle import c_oracle
    _, P, X, r, _, _ = c1
    B = 256
    P, xs, lg, lx = P[:B], r["x"][:B], r["lam_g"][:B], r["lam_x"][:B]
    s = BatchedOCPSolver(10, 4, 0.1)
    s.set_team_waves(waves)
    o = s.solve_batch(_t(P), _t(xs), lam_g0=_t(lg), lam_x0=_t(lx))
    torch.cuda.synchronize()
    state, _ = checker(P, xs, lg, lx, 10, 4)
    ref = c_oracle.solve(P, xs, 10, 4, 0.1, state=state)
    st, it = o["status"].cpu().numpy(), o["iters"].cpu().numpy()
    assert (st == ref["status"]).all()
    # the tolerance of the stateless GPU-vs-oracle comparison (test_gpu_parity.py): 5 of these 256 warm solves have been seen 2 iterations apart (the
    # checker's tube rows differ from the kernel's in the last bits -- c and wd by two codes --, and a warm start at x* sits on the active rows)
    d_it = np.abs(it - ref["iters"])
    print(f"\nwaves {waves}: iterations vs oracle: {int((d_it == 1).sum())} problems 1 apart, {int((d_it == 2).sum())} 2 apart of {B}")
    assert d_it.max() <= 2
    ok = st == 0
    assert _rms_q(o["x"].cpu().numpy()[ok], ref["x"][ok]) < 1e-7
    s.close()


def test_resolve_from_solution_with_its_own_multipliers(c1):
    import torch
    s, P, X, r, _, _ = c1
    o = s.solve_batch(_t(P), _t(r["x"]), out={}, lam_g0=_t(r["lam_g"]), lam_x0=_t(r["lam_x"]))
    o0 = s.solve_batch(_t(P), _t(r["x"]), out={})
    torch.cuda.synchronize()
    ok = r["status"] == 0
    st, it, x = o["status"].cpu().numpy(), o["iters"].cpu().numpy(), o["x"].cpu().numpy()
    assert (st[ok] == 0).all()
    d = np.sqrt(np.mean((x - r["x"]).reshape(-1, 10, 44)[:, :, 8:15] ** 2, axis=(1, 2)))[ok]
    print(f"\nconfigs[1]: mean / max iterations cold {r['iters'][ok].mean():.2f} / {r['iters'][ok].max()}, x* without multipliers "
          f"{o0['iters'].cpu().numpy()[ok].mean():.2f} / {o0['iters'].cpu().numpy()[ok].max()}, x* with multipliers {it[ok].mean():.2f} / {it[ok].max()}; "
          f"{int((d >= 1e-7).sum())} minimisers moved (flat valleys), median {np.median(d):.1e} rad")
    assert np.median(d) < 1e-7 and (d < 1e-7).mean() > 0.9
    assert it[ok].mean() < r["iters"][ok].mean()


def _closed_loop(which, duals, ticks=25):
    from boundmpc_amd import workload
    from boundmpc_amd.bound_mpc import BoundMPC, integrate_joint
    from boundmpc_amd.robot_model import RobotModel
    d6, d7 = np.load(os.path.join(G, f"g6_pack_exp{which}_tick0.npz")), np.load(os.path.join(G, f"g7_closedloop_exp{which}.npz"))
    mk = lambda k: [np.array(v) for v in d6[k]]
    prm = workload.Params(weights=d6["weights_f64"], build=True)
    prm.warm_start_duals = duals
    mpc = BoundMPC(mk("p_via"), mk("r_via"), [mk("p_lower"), mk("p_upper")], [mk("r_lower"), mk("r_upper")], mk("bp1_in"), mk("br1_in"),
                   list(d6["s_in"]), list(d6["e_p_min_in"]), list(d6["e_r_min_in"]), list(d6["e_p_max_in"]), list(d6["e_r_max_in"]),
                   p0=d6["p0fk"].copy(), params=prm)
    rm = RobotModel()
    q, dq, ddq, jerk, v = d6["q0"].copy(), np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(6)
    x_phi_d = np.array([mpc.phi_max[0], 0, 0])
    its, dev = [], 0.0
    for i in range(ticks):
        p_lie, _, _ = rm.forward_kinematics(q, dq)
        traj, _, _, _, iters = mpc.step(q, dq, ddq, p_lie, v, x_phi_d, jerk)
        assert mpc.error_count == 0 and mpc.solver.stats()["success"], (which, i, mpc.solver.stats())
        dev = max(dev, float(np.abs(q - d7["q"][i]).max()))
        its.append(iters)
        jm = np.concatenate((jerk[:, None], traj["dddq"][:, :2]), axis=1)
        q, dq, ddq, p_lie, v = integrate_joint(rm, jm, q, dq, ddq, mpc.dt)[:5]
        jerk = traj["dddq"][:, 0].copy()
    mpc.solver.close(); mpc.batched.close()
    return its, dev


@pytest.mark.parametrize("which", [1, 2])
def test_drop_in_closed_loop_with_the_references_hand_over(which):
    """Both experiments through NlpSolverShim with the reference's hand-over restored: every tick converges, no plan is replayed, the plant stays on
    the fixture's loop (solved to 1e-8 by Ipopt).  Without multipliers the loop stays within 1e-6 rad (test_gpu_parity.py); with them a tick converges
    from another start to the same tolerance, and the plant has been seen 1.2e-6 rad off (experiment 1) -- held here to 1e-5."""
    (with_duals, dev), (without, dev0) = _closed_loop(which, True), _closed_loop(which, False)
    print(f"\nexperiment {which}: iterations per tick with lam_g0 / lam_x0 {with_duals} (mean {np.mean(with_duals):.2f}), "
          f"without {without} (mean {np.mean(without):.2f}); plant vs fixture max {dev:.2e} / {dev0:.2e} rad")
    assert dev < 1e-5 and dev0 < 1e-6


def test_default_paths_unchanged():
    import torch
    from boundmpc_amd import BatchedOCPSolver, NlpSolverShim, _lib
    import ctypes
    d = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))
    s = BatchedOCPSolver(10, 4, 0.1)
    shim = NlpSolverShim(s)
    p, x0 = d["p"][3], d["x0"][3]
    base = shim(x0=x0, p=p)
    for lg, lx in ((0, 0), (np.zeros(430), np.zeros((440, 1))), (None, None), (0.0, np.zeros(440))):
        o = shim(x0=x0, p=p, lam_g0=lg, lam_x0=lx)
        for k in ("x", "g", "lam_g", "lam_x"):
            assert np.array_equal(o[k], base[k])
        assert o["f"] == base["f"]
    assert set(shim.stats()) == {"iter_count", "success", "return_status", "kkt_error"}
    with pytest.raises(ValueError):
        shim(x0=x0, p=p, lam_g0=np.ones(429))
    o = shim(x0=x0, p=p, lam_g0=np.asarray(base["lam_g"]), lam_x0=np.asarray(base["lam_x"]))
    assert shim.stats()["success"]
    # solve_batch without multipliers against a direct bmpc_solve_batch
    P, X = _t(d["p"][:64]), _t(d["x0"][:64])
    a = s.solve_batch(P, X, out={})
    x = torch.empty_like(X); it = torch.empty(64, dtype=torch.int32, device="cuda")
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(s._lib.bmpc_solve_batch(s._h, 64, dp(P), dp(X), dp(x), None, None, None, None, dp(it), None, None,
                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "bmpc_solve_batch")
    torch.cuda.synchronize()
    assert torch.equal(a["x"], x) and torch.equal(a["iters"], it)
    shim.close(); s.close()


def test_hostile_input_and_refused_calls():
    import torch
    import ctypes
    from boundmpc_amd import BatchedOCPSolver, _lib
    d = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))
    B = 8
    s = BatchedOCPSolver(10, 4, 0.1)
    P, X = _t(d["p"][:B]), _t(d["x"][:B])
    lg, lx = np.tile(np.linspace(-3, 3, 430), (B, 1)), np.tile(np.linspace(-2, 2, 440), (B, 1))
    lg[0] = np.nan; lx[1] = np.inf; lx[2] = -np.inf; lg[3] = 1e300; lx[4] = -1e300; lg[5] *= -1; lx[5] *= -1
    o = s.solve_batch(P, X, lam_g0=_t(lg), lam_x0=_t(lx))
    torch.cuda.synchronize()
    st = o["status"].cpu().numpy()
    assert ((st >= 0) & (st <= 3)).all() and torch.isfinite(o["x"]).all() and torch.isfinite(o["state"]).all()
    with pytest.raises(ValueError):
        s.solve_batch(P, X, state=s.new_state(B), lam_g0=_t(lg))
    out = s.new_state(B)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    strm = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = s._lib.bmpc_state_from_multipliers
    assert f(None, B, vp(P), vp(X), None, None, 0.0, vp(out), strm) == 1
    assert f(s._h, -1, vp(P), vp(X), None, None, 0.0, vp(out), strm) == 1
    assert f(s._h, B, None, vp(X), None, None, 0.0, vp(out), strm) == 1
    assert f(s._h, B, vp(P), vp(X), None, None, 0.0, None, strm) == 1
    assert f(s._h, 0, None, None, None, None, 0.0, None, strm) == 0
    h = s._lib.bmpc_solve_batch_host_dual
    assert h(s._h, -1, *([None] * 12)) == 1 and h(None, 1, *([None] * 12)) == 1
    s.close()


def test_cross_stream_ordering_matches_one_stream():
    import torch
    from boundmpc_amd import BatchedOCPSolver, workload
    P, X, _ = workload.make_batch(600, seed=5)
    p, x0 = _t(P), _t(X)

    def run(two):
        s = BatchedOCPSolver(10, 4, 0.1)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        # every launch of the handle waits for the one before it (its event), whatever stream: each reads what the earlier ones wrote
        a = s.solve_batch(p, x0, out={}, stream=s1)
        lg, lx = a["lam_g"], a["lam_x"]
        st = s.state_from_multipliers(p, a["x"], lg, lx, stream=s2 if two else s1)
        b = s.solve_batch(p, a["x"], out={}, stream=s1)
        c = s.solve_batch(p, a["x"], out={}, state=st, stream=s2 if two else s1)
        d = s.solve_batch(p, x0, out={}, stream=s2 if two else s1, lam_g0=lg, lam_x0=lx)
        torch.cuda.synchronize()
        res = [t.cpu().numpy().copy() for t in (st, b["x"], c["x"], c["iters"], d["x"], d["state"])]
        s.close()
        return res

    for u, v in zip(run(False), run(True)):
        assert np.array_equal(u, v)
