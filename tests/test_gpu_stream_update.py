"""GPU: re-planning of closed-loop streams on the device (bmpc_stream_update of the C ABI, StreamBatch.update_device) against the reference's own
update() / step() (fixture G11), against the g++ build of the same kernel text on the same inputs, inside a caller's captured graph, and on a stream
that had lost its plan.  Open-loop comparisons only: the device table and the host table differ in the last bits and a closed loop amplifies that."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def test_replanning_by_the_device_matches_reference_update_g11():
    """tests/test_gpu_stream.py test_replanning_on_the_device_matches_reference_update_g11 with sb.update_device(record) in place of the host's
    sb.update(...): the same quantities at the same tolerances, and the goal the launch writes into the robot record."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream
    from oracle import c_oracle
    from tests.closed_loop import fixture_mpc
    from tests.emu import emu_stream_update as eup
    mpc, d6 = fixture_mpc(1)
    d7 = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))
    d = np.load(os.path.join(G, "g11_update.npz"))
    T_UPD = int(d["t_update"])
    solver = BatchedOCPSolver(10, 4, 0.1)
    sb = bstream.StreamBatch(solver, [mpc])
    xphid = np.array([mpc.phi_max[0], 0, 0])
    assert solver._lib.bmpc_stream_replan_len(solver._h, sb.entries) == bstream.replan_len(4, sb.entries) == 32 + 32 * (sb.entries - 3)
    assert solver._lib.bmpc_stream_replan_len(solver._h, 4) <= 0 and solver._lib.bmpc_stream_replan_len(None, sb.entries) <= 0

    def feed(q, dq, ddq, p_lie, v, jerk, x, p_fix, status):
        sb.set_robot(bstream.robot_record(q, dq, ddq, p_lie, v, xphid, jerk)[None])
        sb.pack(); torch.cuda.synchronize()
        p, x0 = sb.p.cpu().numpy()[0].copy(), sb.x0.cpu().numpy()[0].copy()
        g = c_oracle.eval_fg(p_fix, x, 10, 4, 0.1)[1]
        sb.x.copy_(torch.tensor(x[None])); sb.g.copy_(torch.tensor(g[None])); sb.status.fill_(int(status))
        sb.post(simulate=False); torch.cuda.synchronize()
        return p, x0
    for t in range(T_UPD):
        feed(d7["q"][t], d7["dq"][t], d7["ddq"][t], d7["p_lie"][t], d7["v"][t], d7["jerk"][t], d7["x"][t], d7["p"][t], 0)
    info = sb.update_device(bstream.replan_record(4, sb.entries, *eup.g11_args())[None])
    torch.cuda.synchronize()
    st, rb = sb.state.cpu().numpy()[0], sb.robot.cpu().numpy()[0]
    phi_max = float(st[bstream.SS["PHIMAX"]])
    assert info.cpu().numpy().tolist() == [0] and float(sb.replan[0, 0]) == 0.0
    assert abs(phi_max - float(d["after_update_phi_max"])) < 1e-13
    np.testing.assert_allclose(rb[bstream.RB["XPHID"]:bstream.RB["XPHID"] + 3], [float(d["after_update_phi_max"]), 0.0, 0.0], atol=1e-13, rtol=0)
    np.testing.assert_allclose(st[3:7], d["after_update_phi"], atol=1e-11)
    np.testing.assert_allclose(st[7:10], eup.flip_pi(st[7:10], d["after_update_pr_ref"]), atol=1e-11)
    np.testing.assert_allclose(st[10:13], d["after_update_iw_ref"], atol=1e-11)
    xphid = np.array([phi_max, 0, 0])
    mask = d6["p_defined_mask"]
    for i in range(len(d["x"])):
        p, x0 = feed(d["q"][i], d["dq"][i], d["ddq"][i], d["p_lie"][i], d["v"][i], d["jerk"][i], d["x"][i], d["p"][i], int(d["status"][i]))
        np.testing.assert_allclose(p[mask], d["p"][i][mask], atol=5e-11, rtol=1e-11, err_msg=f"p, tick {i} after update")
        np.testing.assert_allclose(x0, d["x0"][i], atol=1e-11, err_msg=f"x0, tick {i} after update")
        st = sb.state.cpu().numpy()[0]
        td, _ = bstream.unpack_traj(sb.traj.cpu().numpy()[0], 10)
        np.testing.assert_allclose(td["q"], d["traj_q"][i], atol=1e-11)
        assert abs(bstream.phi(st) - d["phi_current"][i]) < 1e-11 and int(st[0]) == int(d["sector"][i])
        np.testing.assert_allclose(st[10:13], d["iw_ref"][i], atol=1e-11)
    # a missing array, an empty batch and a table shorter than S + 1 entries are argument errors, not launches
    from boundmpc_amd.solver import _ptr
    args = [1, _ptr(sb.replan), _ptr(sb.path), sb.entries, _ptr(sb.state), _ptr(sb.robot), _ptr(sb.replan_info), 1]
    for i in (1, 2, 4):
        assert solver._lib.bmpc_stream_update(solver._h, *[None if j == i else a for j, a in enumerate(args)], None) == 1
    assert solver._lib.bmpc_stream_update(solver._h, 0, *args[1:], None) == 1 and solver._lib.bmpc_stream_update(solver._h, *args[:3], 4, *args[4:], None) == 1
    assert solver._lib.bmpc_stream_update(solver._h, *args[:5], None, None, 1, None) == 0      # robot and info may be missing
    torch.cuda.synchronize()
    sb.close(); solver.close()


@pytest.mark.parametrize("N,S", [(10, 4), (5, 2), (12, 6)])
def test_device_update_equals_cpu_build_of_the_same_text(N, S):
    """Eight streams in one launch: five flagged (n = 2, 3, 5, 8 and one with nb < n), two unflagged, one invalid record.  Flagged: table and
    state within 1e-11 of tests/emu's g++ build of csrc/bmpc_stream_update.inl on the same inputs; the others bit-equal to before; info and the
    cleared flags; a second launch with no flag raised changes nothing."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload
    from boundmpc_amd.bound_mpc import BoundMPC
    from tests.closed_loop import Oracle
    from tests.emu import emu_stream_update as eup
    rng = np.random.default_rng(100 * N + S)
    long_path = eup.random_path(rng, 8)
    keys = ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min", "e_p_max", "e_r_max")
    mpc = BoundMPC(p0=long_path["p0"].copy(), params=workload.Params(n=N, dt=0.1, nr_segs=S), solver=Oracle(), **{k: long_path[k] for k in keys})
    solver = BatchedOCPSolver(N, S, 0.1)
    sb = bstream.StreamBatch(solver, [mpc] * 8)
    entries = sb.entries
    assert entries == 8 + S - 1
    shapes = [dict(n=2), dict(n=3, vanish_first=True), dict(n=5), dict(n=8, vanish_later=True), dict(n=5, nb=2), dict(n=4), dict(n=6), dict(n=3)]
    recs = np.stack([bstream.replan_record(S, entries, *eup.args_of(eup.random_path(rng, **kw))) for kw in shapes])
    recs[5, 0] = recs[6, 0] = 0.0                     # unflagged
    recs[7, bstream.RP["N"]] = entries - S + 2        # one via point more than the table holds
    flagged, others = [0, 1, 2, 3, 4], [5, 6, 7]
    state0 = np.stack([eup.random_state(rng, N, error_count=(N if b == 2 else b % 3), has_prev=bool(b % 2)) for b in range(8)])
    path0, robot0 = rng.normal(size=(8, entries, 48)), rng.normal(size=(8, bstream.RB["LEN"]))
    sb.state.copy_(torch.tensor(state0)); sb.path.copy_(torch.tensor(path0)); sb.robot.copy_(torch.tensor(robot0))
    info = sb.update_device(recs)
    torch.cuda.synchronize()
    got = [a.cpu().numpy().copy() for a in (sb.path, sb.state, sb.robot)]
    assert info.cpu().numpy().tolist() == [0, 0, 0, 0, 0, 0, 0, 1] and (sb.replan[:, 0] == 0.0).all() and np.array_equal(sb.replan.cpu().numpy()[:, 1:], recs[:, 1:])
    for b in flagged:
        i_cpu, _, T, ss, rb = eup.stream_update(N, S, recs[b], path0[b], state0[b], robot0[b])
        assert i_cpu == 0
        eup.assert_close(got[0][b], got[1][b], T, ss, 1e-11, what=f"stream {b} {shapes[b]}")
        np.testing.assert_allclose(got[2][b], rb, atol=1e-11, rtol=0)
        assert got[1][b][bstream.SS["NENT"]] == shapes[b]["n"] + S - 1 and got[1][b][bstream.ss_updated(N)] == 1.0
    assert got[1][2][bstream.SS["ERRCNT"]] == N - 1
    for b in others:
        assert np.array_equal(got[0][b], path0[b]) and np.array_equal(got[1][b], state0[b]) and np.array_equal(got[2][b], robot0[b]), b
    info = sb.update_device(sb.replan)                # no flag raised: nothing changes
    torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [0] * 8
    for a, was in zip((sb.path, sb.state, sb.robot), got):
        assert np.array_equal(a.cpu().numpy(), was)
    sb.close(); solver.close()


def test_update_inside_a_captured_graph_equals_direct_launches():
    """Twins of four workload streams over 12 converged ticks: one calls update_device + tick directly, the other replays ONE graph the caller
    captured around the same two calls.  Both raise the flags of streams 1 and 3 in the record buffer on the device after tick 5.  States, plant
    records and trajectories are bit-equal after every tick; phi_max of the re-planned streams changes at tick 6, that of the others never."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload
    from boundmpc_amd.robot_model import RobotModel
    mpcs, recs = workload.make_streams(4, seed=3)
    rm = RobotModel()
    records = []
    for b in range(4):                                 # the other experiment's path from the stream's start pose, measured state: at rest there
        p0fk = recs[b][bstream.RB["P"]:bstream.RB["P"] + 6]
        path = workload.experiment2_path(p0fk)
        records.append(bstream.replan_record(4, 8, *[path[k] for k in ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min",
                                                                        "e_p_max", "e_r_max")], p0fk, np.zeros(6), np.zeros(6), np.zeros(6), p0fk, mpcs[b].weights))
    records = np.stack(records); records[:, 0] = 0.0
    twins = []
    for _ in range(2):
        solver = BatchedOCPSolver(10, 4, 0.1)
        sb = bstream.StreamBatch(solver, mpcs)
        sb.set_robot(recs)
        twins.append((solver, sb))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = None
    phimax = []
    with torch.cuda.stream(side):
        for solver, sb in twins:
            assert sb.entries == 8
            sb.update_device(records)                  # allocates the record buffer, re-plans nothing
            sb.tick(simulate=True)                     # tick 0, direct on both
        side.synchronize()
        for t in range(1, 12):
            if t == 6:
                for _, sb in twins:
                    sb.replan[[1, 3], 0] = 1.0
            sb = twins[0][1]
            sb.update_device(sb.replan); sb.tick(simulate=True)
            sb = twins[1][1]
            if graph is None:
                side.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
                    sb.update_device(sb.replan); sb.tick(simulate=True)
            graph.replay()
            side.synchronize()
            a, b = twins[0][1], twins[1][1]
            for x, y, what in ((a.state, b.state, "state"), (a.robot, b.robot, "robot"), (a.traj, b.traj, "traj"), (a.path, b.path, "path"), (a.replan, b.replan, "replan")):
                assert torch.equal(x, y) or np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True), f"tick {t}: {what}"
            assert (a.replan[:, 0] == 0.0).all() and a.replan_info.cpu().numpy().tolist() == [0, 0, 0, 0]
            phimax.append(b.state[:, bstream.SS["PHIMAX"]].cpu().numpy().copy())
    phimax = np.stack(phimax)                          # rows: ticks 1..11
    assert (phimax[:5] == phimax[0]).all() and (phimax[5:] == phimax[5]).all()
    assert (phimax[5, [1, 3]] != phimax[0, [1, 3]]).all() and (phimax[5, [0, 2]] == phimax[0, [0, 2]]).all()
    assert (twins[1][1].state[[1, 3], bstream.ss_updated(10)] == 1.0).all() and (twins[1][1].state[[0, 2], bstream.ss_updated(10)] == 0.0).all()
    del graph
    torch.cuda.synchronize()
    for solver, sb in twins:
        sb.close(); solver.close()


def test_a_stream_that_lost_its_plan_is_solved_again_after_update_device():
    """Error count N: the fused tick skips the stream (status 3, 0 iterations).  After update_device (error count N - 1, cold start on the new
    path) the next fused tick solves it."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload
    N = 10
    mpcs, recs = workload.make_streams(2, seed=3)
    solver = BatchedOCPSolver(N, 4, 0.1)
    sb = bstream.StreamBatch(solver, mpcs)
    sb.set_robot(recs)
    sb.state[1, bstream.SS["ERRCNT"]] = float(N)
    sb.tick(simulate=True); torch.cuda.synchronize()
    assert sb.status.cpu().numpy().tolist()[1] == 3 and sb.iters.cpu().numpy().tolist()[1] == 0 and sb.iters.cpu().numpy().tolist()[0] > 0
    assert not bool(sb.has_plan()[1])
    p0fk = recs[1][bstream.RB["P"]:bstream.RB["P"] + 6]
    path = workload.experiment1_path(p0fk)
    rec = bstream.replan_record(4, sb.entries, *[path[k] for k in ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min", "e_p_max",
                                                                    "e_r_max")], p0fk, np.zeros(6), np.zeros(6), np.zeros(6), p0fk, mpcs[1].weights)
    records = np.zeros((2, rec.shape[0])); records[1] = rec
    info = sb.update_device(records)
    sb.tick(simulate=True); torch.cuda.synchronize()
    assert info.cpu().numpy().tolist() == [0, 0]
    assert sb.iters.cpu().numpy().tolist()[1] > 0 and sb.status.cpu().numpy().tolist()[1] != 3 and bool(sb.has_plan()[1])
    sb.close(); solver.close()
