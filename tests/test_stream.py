"""Device-side tick of BoundMPC.step(): csrc/bmpc_stream.inl compiled for the CPU (tests/emu) and driven
in closed loop with the CPU oracle as the solver, against
  (i) the committed closed-loop fixtures G7 (p, x0, trajectory and phi-state of every tick, produced by the REFERENCE's own
      step()/compute_return_data -- tests/golden/make_golden.py), and
 (ii) the host mirror boundmpc_amd.bound_mpc.BoundMPC on a synthetic stream, including the failure fallback."""
import os

import numpy as np
import pytest

from boundmpc_amd import stream as bstream, workload
from boundmpc_amd.bound_mpc import integrate_joint
from boundmpc_amd.robot_model import RobotModel
from oracle import c_oracle
from tests.closed_loop import Oracle, cpu_mirror_loop, fixture_mpc, fixture_robot_record, stream_arrays
from tests.emu import emu

G = os.path.join(os.path.dirname(__file__), "golden")


def _same_rotation(rv_a, rv_b, tol):
    """Rotation vectors compared as rotations: at angle pi the vectors v and -v are the same rotation and the sign is round-off."""
    from scipy.spatial.transform import Rotation as R
    np.testing.assert_allclose(R.from_rotvec(rv_a).as_matrix(), R.from_rotvec(rv_b).as_matrix(), atol=tol)


@pytest.mark.parametrize("which,ticks", [(1, 155), (2, 59)])
def test_stream_closed_loop_retraces_reference_fixture(which, ticks):
    """pack -> (oracle) solve -> post with the plant simulation, nothing else: every tick's p and x0 equal what the reference's
    step() assembled, the trajectory and the advanced phi / rotation-reference state equal compute_return_data's."""
    mpc, d6 = fixture_mpc(which, Oracle())
    d7 = np.load(os.path.join(G, f"g7_closedloop_exp{which}.npz"))
    mask = d6["p_defined_mask"]        # row S of a4..a0 is uninitialised memory in the reference; defined here as row S-1
    worst_p = worst_x0 = 0.0
    for c in cpu_mirror_loop(mpc, fixture_robot_record(mpc, d6), ticks, solve=Oracle().solve):
        t, p, x0, ss = c["t"], c["p"], c["x0"], c["ss"]
        np.testing.assert_allclose(c["q"], d7["q"][t], atol=2e-6)
        worst_p = max(worst_p, np.abs(p - d7["p"][t])[mask].max()); worst_x0 = max(worst_x0, np.abs(x0 - d7["x0"][t]).max())
        td, fl = bstream.unpack_traj(c["traj"], 10)
        assert fl["success"] and fl["n_valid"] == 10 and not fl["using_previous"]
        for k in ("q", "dq", "ddq", "dddq", "p", "v", "a", "phi", "dphi", "ddphi", "dddphi"):
            # the loop feeds the solver's 1e-8-tolerance round-off back into the next problem; jerks are the weakly determined
            # variables (w_jerk = 1e-4), everything integrated from them is smoother
            tol = 2e-3 if k in ("dddq", "dddphi") else (2e-4 if k in ("ddq", "a", "ddphi") else 2e-5)
            np.testing.assert_allclose(td[k], d7["traj_" + k][t], atol=tol, err_msg=f"tick {t} {k}")
        assert abs(bstream.phi(ss) - d7["phi_current"][t]) < 1e-6
        _same_rotation(ss[7:10], d7["pr_ref"][t], 1e-6)
        np.testing.assert_allclose(ss[10:13], d7["iw_ref"][t], atol=1e-6)
        assert int(ss[0]) == int(d7["sector"][t])
    # the closed loop amplifies solver round-off (tol 1e-8) from tick to tick; per tick the packing itself is exact (next test)
    assert worst_p < 2e-3 and worst_x0 < 2e-3      # dominated by the jerk entries (jerk_current in p, shifted jerks in x0)


@pytest.mark.parametrize("which", [1, 2])
def test_stream_pack_is_exact_given_the_reference_state(which):
    """Open loop: feed the recorded robot state and the recorded previous solution of each tick -> p and x0 to round-off."""
    mpc, d6 = fixture_mpc(which, Oracle())
    d7 = np.load(os.path.join(G, f"g7_closedloop_exp{which}.npz"))
    T, ss = stream_arrays(mpc, 10)
    xphid = np.array([mpc.phi_max[0], 0, 0])
    mask = d6["p_defined_mask"]
    n = d7["p"].shape[0]
    for t in range(n):
        rb = bstream.robot_record(d7["q"][t], d7["dq"][t], d7["ddq"][t], d7["p_lie"][t], d7["v"][t], xphid, d7["jerk"][t])
        p, x0 = emu.stream_pack(10, 4, T, ss, rb)
        np.testing.assert_allclose(p[mask], d7["p"][t][mask], atol=2e-11, rtol=1e-11, err_msg=f"tick {t}")
        np.testing.assert_allclose(x0, d7["x0"][t], atol=1e-13)
        g = c_oracle.eval_fg(d7["p"][t], d7["x"][t], 10, 4, 0.1)[1]
        emu.stream_post(10, 4, 0.1, T, ss, rb.copy(), d7["x"][t], g, int(d7["status"][t]), simulate=False)
        assert abs(bstream.phi(ss) - d7["phi_current"][t]) < 1e-12
        _same_rotation(ss[7:10], d7["pr_ref"][t], 1e-11)
        np.testing.assert_allclose(ss[10:13], d7["iw_ref"][t], atol=1e-12)


def test_stream_matches_host_mirror_with_failures():
    """Synthetic stream (random start, workload generator), solver failing at ticks 3,4 and 9: the device-side state machine
    (error count, fallback to the previous plan, shortened trajectories) follows the host mirror's."""
    q0 = workload.random_q0(3, seed=5)[2]
    fails = (3, 4, 9)
    mpc, p0fk = workload.make_mpc(q0, solver=Oracle(fails))
    ref, _ = workload.make_mpc(q0, solver=Oracle())
    rm = RobotModel()
    q, dq, ddq, jerk, v = q0.copy(), np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(6)
    x_phi_d = np.array([mpc.phi_max[0], 0, 0])
    for c in cpu_mirror_loop(ref, bstream.robot_record(q, dq, ddq, p0fk, v, x_phi_d, jerk), 14, solve=Oracle(fails).solve):
        t, ss, rb = c["t"], c["ss"], c["rb"]
        p_lie = rm.forward_kinematics(q, dq)[0]
        w0, params, _ = mpc.pack(q, dq, ddq, p_lie, v, x_phi_d, jerk)
        # undo the side effects of the extra pack() call?  none: pack() only reads/updates the window, which step() repeats identically
        traj, _, _, _, _ = mpc.step(q, dq, ddq, p_lie, v, x_phi_d, jerk)
        # two independent closed loops: each solve's 1e-8-level freedom in the jerks feeds the next tick
        np.testing.assert_allclose(c["p"], params, atol=2e-6, rtol=1e-9, err_msg=f"tick {t}")
        np.testing.assert_allclose(c["x0"], np.array(w0), atol=2e-6)
        td, fl = bstream.unpack_traj(c["traj"], 10)
        assert int(ss[bstream.SS["ERRCNT"]]) == mpc.error_count
        assert fl["using_previous"] == (t in fails)
        assert fl["n_valid"] == 10 - mpc.error_count
        for k in ("q", "dq", "ddq", "dddq", "p", "v", "a", "phi", "dphi", "ddphi", "dddphi"):
            np.testing.assert_allclose(td[k], traj[k], atol=2e-5 if k in ("dddq", "dddphi") else 2e-6, err_msg=f"tick {t} {k}")
        jm = np.concatenate((jerk[:, None], traj["dddq"][:, :2]), axis=1)
        q, dq, ddq, p_lie, v = integrate_joint(rm, jm, q, dq, ddq, mpc.dt)[:5]
        jerk = traj["dddq"][:, 0].copy()
        np.testing.assert_allclose(rb[:7], q, atol=1e-7)
        np.testing.assert_allclose(rb[21:27], p_lie, atol=1e-7)


def test_second_time_derivative_of_the_jacobian_g1():
    """The closed form of d2/dt2 J_v for the geometric chain (csrc/bmpc_stream.inl, needed for the Cartesian jerk of the previous plan
    after a re-planning) against the reference's Maple-generated ddjacobian_fk (RobotModel.py:565-1053) on 256 random states."""
    d = np.load(os.path.join(G, "g1_kinematics.npz"))
    for i in range(len(d["q"])):
        np.testing.assert_allclose(emu.jacobian_lin_ddot(d["q"][i], d["dq"][i], d["ddq"][i]), d["ddjacobian_fk"][i][:3], atol=2e-14)


def test_fk_motion_against_the_references_kinematics_g1():
    """fk_motion (csrc/bmpc_stream.inl: the post-processing's one-pass pose / velocity / acceleration / jerk) against the reference's own
    kinematics on the 256 random states of fixture G1: pose = fk, v = J dq, a = J ddq + dJ dq with the Maple-generated jacobian_fk /
    djacobian_fk values, and the linear jerk rows J u + dJ ddq + ddJ dq with its ddjacobian_fk (RobotModel.py:254-1053)."""
    d = np.load(os.path.join(G, "g1_kinematics.npz"))
    rng = np.random.default_rng(0)
    for i in range(len(d["q"])):
        q, dq, ddq = d["q"][i], d["dq"][i], d["ddq"][i]
        u = rng.uniform(-5, 5, 7)
        p, v, a, jk = emu.fk_motion(q, dq, ddq, u)
        J, dJ, ddJ = d["jacobian_fk"][i], d["djacobian_fk"][i], d["ddjacobian_fk"][i]
        np.testing.assert_allclose(p[:3], d["fk_pos"][i], atol=1e-14)
        np.testing.assert_allclose(p, d["fk"][i], atol=1e-13)      # pose [position | rotation vector] of RobotModel.forward_kinematics
        np.testing.assert_allclose(v, J @ dq, atol=1e-13)
        np.testing.assert_allclose(a, J @ ddq + dJ @ dq, atol=1e-12)
        np.testing.assert_allclose(jk, (J @ u + dJ @ ddq + ddJ @ dq)[:3], atol=1e-11)


def test_stream_replanning_matches_reference_update_g11():
    """Re-planning on the stream functions: the recorded experiment-1 loop up to the tick of the update, `apply_update` (the state part
    of BoundMPC.update), then the ticks after it -- whose warm start goes through the re-projection branch with the Cartesian
    derivatives of the previous plan kept by stream_post -- against what the REFERENCE's own update()/step() produced (fixture G11)."""
    mpc, d6 = fixture_mpc(1, Oracle())
    d7 = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))
    d = np.load(os.path.join(G, "g11_update.npz"))
    T_UPD = int(d["t_update"])
    T, ss = stream_arrays(mpc, 10)
    xphid = np.array([mpc.phi_max[0], 0, 0])
    for t in range(T_UPD):          # open loop over the recorded ticks (states and solutions of G7)
        rb = bstream.robot_record(d7["q"][t], d7["dq"][t], d7["ddq"][t], d7["p_lie"][t], d7["v"][t], xphid, d7["jerk"][t])
        emu.stream_pack(10, 4, T, ss, rb)
        g = c_oracle.eval_fg(d7["p"][t], d7["x"][t], 10, 4, 0.1)[1]
        emu.stream_post(10, 4, 0.1, T, ss, rb, d7["x"][t], g, 0, simulate=False)
    L = lambda k: [np.array(v) for v in d["upd_" + k]]
    T2, M2 = bstream.apply_update(ss, 10, 4, L("p_via"), L("r_via"), [L("p_lower"), L("p_upper")], [L("r_lower"), L("r_upper")], L("bp1"), L("br1"),
                                  list(d["upd_s"]), list(d["upd_e_p_min"]), list(d["upd_e_r_min"]), list(d["upd_e_p_max"]), list(d["upd_e_r_max"]),
                                  d["upd_p"], d["upd_v"], d["upd_a"], d["upd_jerk"], d["upd_p"], d["weights"])
    np.testing.assert_allclose(ss[3:7], d["after_update_phi"], atol=1e-13)
    np.testing.assert_allclose(ss[7:10], d["after_update_pr_ref"], atol=1e-12)
    np.testing.assert_allclose(ss[10:13], d["after_update_iw_ref"], atol=1e-12)
    assert abs(ss[bstream.SS["PHIMAX"]] - float(d["after_update_phi_max"])) < 1e-13
    xphid = np.array([ss[bstream.SS["PHIMAX"]], 0, 0])
    mask = d6["p_defined_mask"]
    for i in range(len(d["x"])):
        rb = bstream.robot_record(d["q"][i], d["dq"][i], d["ddq"][i], d["p_lie"][i], d["v"][i], xphid, d["jerk"][i])
        p, x0 = emu.stream_pack(10, 4, T2, ss, rb)
        np.testing.assert_allclose(p[mask], d["p"][i][mask], atol=5e-11, rtol=1e-11, err_msg=f"p, tick {i} after update")
        np.testing.assert_allclose(x0, d["x0"][i], atol=1e-11, err_msg=f"x0, tick {i} after update")
        g = c_oracle.eval_fg(d["p"][i], d["x"][i], 10, 4, 0.1)[1]
        tr = emu.stream_post(10, 4, 0.1, T2, ss, rb, d["x"][i], g, int(d["status"][i]), simulate=False)
        td, fl = bstream.unpack_traj(tr, 10)
        np.testing.assert_allclose(td["q"], d["traj_q"][i], atol=1e-12)
        np.testing.assert_allclose(td["phi"], d["traj_phi"][i], atol=1e-12)
        assert abs(bstream.phi(ss) - d["phi_current"][i]) < 1e-12 and int(ss[0]) == int(d["sector"][i])
        _same_rotation(ss[7:10], d["pr_ref"][i], 1e-11)
        np.testing.assert_allclose(ss[10:13], d["iw_ref"][i], atol=1e-12)


@pytest.mark.parametrize("N,S", [(5, 2), (8, 3), (20, 4), (6, 5), (12, 6)])
def test_stream_functions_other_horizons_and_windows_g12(N, S):
    """stream_pack / stream_post for other (n, nr_segs) against the reference's own step() (fixture G12), open loop over its ticks."""
    d = np.load(os.path.join(G, "g12_pack_other_sizes.npz"))
    k = f"n{N}s{S}_"
    dt, mask = float(d[k + "dt"]), d[k + "mask"]
    mpc, _ = fixture_mpc(2, n=N, dt=dt, nr_segs=S, weights=d["weights"])
    T, ss = stream_arrays(mpc, N)
    xphid = np.array([mpc.phi_max[0], 0, 0])
    for i in range(len(d[k + "x"])):
        rb = bstream.robot_record(d[k + "q"][i], d[k + "dq"][i], d[k + "ddq"][i], d[k + "p_lie"][i], d[k + "v"][i], xphid, d[k + "jerk"][i])
        p, x0 = emu.stream_pack(N, S, T, ss, rb)
        np.testing.assert_allclose(p[mask], d[k + "p"][i][mask], atol=2e-11, rtol=1e-11, err_msg=f"tick {i}")
        np.testing.assert_allclose(x0, d[k + "x0"][i], atol=1e-13)
        g = c_oracle.eval_fg(d[k + "p"][i], d[k + "x"][i], N, S, dt)[1]
        tr = emu.stream_post(N, S, dt, T, ss, rb.copy(), d[k + "x"][i], g, 0, simulate=False)
        td, fl = bstream.unpack_traj(tr, N)
        np.testing.assert_allclose(td["q"], d[k + "traj_q"][i], atol=1e-12)
        np.testing.assert_allclose(td["p"], d[k + "traj_p"][i], atol=1e-11)
        assert abs(bstream.phi(ss) - d[k + "phi_current"][i]) < 1e-12
        _same_rotation(ss[7:10], d[k + "pr_ref"][i], 1e-11)


def test_realtime_continuation_rule_of_stream_pack():
    """Real-time mode (flag bit 1 of stream_post, not in the reference): an iteration-capped iterate that fails the acceptance rule is not
    applied -- the plant replays the accepted plan -- and the NEXT warm start continues from the rejected iterate when stream_pack is given it
    (bmpc_stream_pack_rt / the fused and the unfused tick), while plain stream_pack (xlast = NULL) restarts from the last accepted plan as the
    reference does (BoundMPC.py:322-375,468-489).  A numerical failure (status 3) is never continued from."""
    N = 10
    (mpc,), (rb,) = (a[1:] for a in workload.make_streams(3, seed=7, take=2))
    T, ss = stream_arrays(mpc, N)
    sol = Oracle()
    for t in range(3):      # three accepted ticks (converged solves)
        p, x0 = emu.stream_pack(N, 4, T, ss, rb)
        x, g, st, _ = sol.solve(p, x0)
        emu.stream_post(N, 4, 0.1, T, ss, rb, x, g, st, simulate=True, flags=2)
    accepted = ss[bstream.SS["PREV"]:bstream.SS["PREV"] + 44 * N].copy()
    # tick 3: a capped iterate (status 1) with a large constraint violation -> rejected, previous plan replayed
    p, x0 = emu.stream_pack(N, 4, T, ss, rb)
    x, g, st, _ = sol.solve(p, x0)
    x_bad = x + 1e-2 * np.random.default_rng(0).standard_normal(x.shape); g_bad = g.copy(); g_bad[:36] += 1e-2
    tr = emu.stream_post(N, 4, 0.1, T, ss, rb, x_bad, g_bad, 1, simulate=True, flags=2, rt_tol=1e-4)
    _, fl = bstream.unpack_traj(tr, N)
    assert fl["using_previous"] and int(ss[bstream.SS["ERRCNT"]]) == 1
    np.testing.assert_array_equal(ss[bstream.SS["PREV"]:bstream.SS["PREV"] + 44 * N], accepted)      # the accepted plan stays the plan
    assert ss[bstream.ss_updated(N) + 1] == 1.0
    shift = lambda a: np.concatenate([a.reshape(N, 44)[1:], a.reshape(N, 44)[-1:]]).ravel()
    ss_a, ss_b = ss.copy(), ss.copy()
    _, x0_ref = emu.stream_pack(N, 4, T, ss_a, rb)                    # reference rule: from the accepted plan
    _, x0_rt = emu.stream_pack(N, 4, T, ss_b, rb, xlast=x_bad)        # real-time rule: from the rejected iterate
    np.testing.assert_array_equal(x0_ref, shift(accepted))
    np.testing.assert_array_equal(x0_rt, shift(x_bad))
    # status 3 clears the continuation word: both rules restart from the accepted plan
    ss_c = ss.copy()
    emu.stream_post(N, 4, 0.1, T, ss_c, rb.copy(), x_bad, g_bad, 3, simulate=True, flags=2, rt_tol=1e-4)
    assert ss_c[bstream.ss_updated(N) + 1] == 0.0
    _, x0_c = emu.stream_pack(N, 4, T, ss_c, rb, xlast=x_bad)
    np.testing.assert_array_equal(x0_c, shift(accepted))


def test_realtime_acceptance_counts_the_variable_bounds():
    """Real-time mode: a capped iterate whose g passes the rule but whose plan leaves a joint limit is NOT applied (the reference's rule looks at
    g only -- Ipopt iterates satisfy the variable bounds by construction; an iteration-capped interior-point iterate of this solver need not)."""
    N = 10
    (mpc,), (rb,) = (a[1:] for a in workload.make_streams(3, seed=7, take=2))
    T, ss = stream_arrays(mpc, N)
    sol = Oracle()
    p, x0 = emu.stream_pack(N, 4, T, ss, rb)
    x, g, st, _ = sol.solve(p, x0)
    emu.stream_post(N, 4, 0.1, T, ss, rb, x, g, st, simulate=True, flags=2)
    p, x0 = emu.stream_pack(N, 4, T, ss, rb)
    x, g, st, _ = sol.solve(p, x0)
    qlim = np.array(RobotModel().q_lim_upper)
    # q_2 of stage 3 beyond its limit; just inside; inside the 1e-9 slack of the solver's own bound rows (a converged iterate with an active bound sits
    # there); just outside it; a jerk beyond 35; a NaN entry (must FAIL the test, not pass it)
    for bad_col, amount, applied in ((8 + 1, 1e-2, False), (8 + 1, -1e-9, True), (8 + 1, 5e-10, True), (8 + 1, 1e-8, False), (0, 1.0, False), (8 + 1, np.nan, False)):
        xb = x.reshape(N, 44).copy()
        xb[3, bad_col] = (qlim[bad_col - 8] if bad_col >= 8 else 35.0) + amount
        tr = emu.stream_post(N, 4, 0.1, T, ss.copy(), rb.copy(), xb.ravel(), g, 1, simulate=True, flags=2, rt_tol=1e-4)
        _, fl = bstream.unpack_traj(tr, N)
        assert fl["success"] == applied, (bad_col, amount, fl)
        # the reference's own rule (flags bit 1 off) does not look at x: the same iterate passes on its g
        tr = emu.stream_post(N, 4, 0.1, T, ss.copy(), rb.copy(), xb.ravel(), g, 1, simulate=True, flags=0)
        assert bstream.unpack_traj(tr, N)[1]["success"]


def test_stream_functions_at_the_longest_horizons_match_the_host_mirror():
    """stream_pack / stream_post beyond 32 stages (round 4: the role map of stream_post follows the horizon): closed loop of the device
    functions against the host mirror (which fixture G12 pins against the reference for other (n, nr_segs)) at N = 36, with one forced failure."""
    N = 36
    q0 = workload.random_q0(3, seed=11)[0]
    Orc = lambda fail_at=(): Oracle(fail_at, N=N, nthreads=4)
    fails = (2,)
    mpc, p0fk = workload.make_mpc(q0, N=N, solver=Orc(fails))
    ref, _ = workload.make_mpc(q0, N=N, solver=Orc())
    rm = RobotModel()
    q, dq, ddq, jerk, v = q0.copy(), np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(6)
    x_phi_d = np.array([mpc.phi_max[0], 0, 0])
    for c in cpu_mirror_loop(ref, bstream.robot_record(q, dq, ddq, p0fk, v, x_phi_d, jerk), 4, N=N, solve=Orc(fails).solve):
        t, ss, rb = c["t"], c["ss"], c["rb"]
        p_lie = rm.forward_kinematics(q, dq)[0]
        traj, _, _, _, _ = mpc.step(q, dq, ddq, p_lie, v, x_phi_d, jerk)
        td, fl = bstream.unpack_traj(c["traj"], N)
        assert int(ss[bstream.SS["ERRCNT"]]) == mpc.error_count and fl["using_previous"] == (t in fails) and fl["n_valid"] == N - mpc.error_count
        for k in ("q", "dq", "p", "v", "phi", "dphi"):
            np.testing.assert_allclose(td[k], traj[k], atol=5e-5, err_msg=f"tick {t} {k}")      # two closed loops of 36-stage solves (tol 1e-8 each)
        jm = np.concatenate((jerk[:, None], traj["dddq"][:, :2]), axis=1)
        q, dq, ddq, p_lie, v = integrate_joint(rm, jm, q, dq, ddq, mpc.dt)[:5]
        jerk = traj["dddq"][:, 0].copy()
        np.testing.assert_allclose(rb[:7], q, atol=1e-6)


def test_level_rule_of_the_pack_and_held_barrier_level_in_oracle_and_kernel_text():
    """Round 6, the barrier level that sets itself: (a) the CPU build of stream_pack writes clamp(c (phi_max - phi), lo, hi) into the mu slot of a WARM
    dual state and leaves a cold one alone; (b) with hold_mu the solve stays on the level it starts on -- the oracle and the kernel text (lane emulator)
    take the same iterations to the same point and hand the level back unchanged."""
    from boundmpc_amd import stream as bstream, workload
    N, S, H = 10, 4, 0.1
    (mpc,), (rb,) = (a[1:] for a in workload.make_streams(4, seed=3, take=2))
    T, ss = stream_arrays(mpc, N)
    dist = float(mpc.phi_max[0] - bstream.phi(ss))
    for mu0, rule, want in ((0.0, (0.02, 0.01, 0.1), 0.0), (0.05, (0.02, 0.01, 0.1), min(max(0.02 * dist, 0.01), 0.1)), (0.05, (1e-4, 0.01, 0.1), 0.01),
                            (0.05, (0.0, 0.0, 0.0), 0.05)):
        dual = np.zeros(c_oracle.state_len(N)); dual[57 * N] = mu0
        p, x0 = emu.stream_pack(N, S, T, ss.copy(), rb, dual=dual, level_rule=rule)
        assert abs(bstream.level(dual, N) - want) < 1e-15, (mu0, rule, dual[57 * N], want)
    # (b) one solve on a held level from a warm state: oracle == kernel text
    P, X, _ = workload.make_batch(4, seed=0)
    for level in (0.05, 0.02):
        kw = dict(tol=1e-3, max_iter=6, mu_init=0.1, mu_warm=0.01, mu_min_fac=10.0, hold_mu=1)
        sa, sb_ = np.zeros((4, c_oracle.state_len(N))), np.zeros((4, c_oracle.state_len(N)))
        sa[:, 57 * N] = level; sb_[:, 57 * N] = level; sa[:, :57 * N] = 1.0; sb_[:, :57 * N] = 1.0
        a = c_oracle.solve(P, X, N, S, H, opts=c_oracle.default_opts(**kw), nthreads=2, state=sa)
        b = emu.solve(P, X, N, S, H, opts=emu.default_opts(**kw), nthreads=2, state=sb_)
        assert (a["status"] == 1).all() and (b["status"] == 1).all() and (a["iters"] == 6).all() and (b["iters"] == 6).all()      # `tol` never fires on a held level
        assert np.allclose(sa[:, 57 * N], level) and np.allclose(sb_[:, 57 * N], level)
        assert np.abs(a["x"] - b["x"]).max() < 1e-8
        kw["hold_mu"] = 0
        c = c_oracle.solve(P, X, N, S, H, opts=c_oracle.default_opts(**kw), nthreads=2, state=sa.copy())
        assert np.abs(c["x"] - a["x"]).max() > 1e-6      # without the hold the barrier walks down: another iterate
