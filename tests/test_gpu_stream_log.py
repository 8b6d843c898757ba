"""GPU: the logging records of BoundMPC.step() from the device (bmpc_stream_log of the C ABI, StreamBatch.log), against the reference's own
dictionaries (fixture G10), against the g++ build of the same kernel text on the same inputs, and behind the fused tick and its graph replay."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


def _cpu_rows(sb, N, S, h):
    """the CPU build of the kernel text fed with the GPU's own (path, sstate, p, traj), row by row"""
    from tests.emu import emu_stream_log as elog
    path, ss, p, traj = (a.cpu().numpy() for a in (sb.path, sb.state, sb.p, sb.traj))
    return np.stack([elog.stream_log(N, S, h, path[b], ss[b], p[b], traj[b]) for b in range(sb.B)])


def test_device_log_equals_the_references_dictionaries_g10():
    """Four streams -- experiment 1 and 2, each with and without the forced solver failure -- open loop over the recorded ticks with
    sb.pack() / sb.post() on the recorded x, g and status, sb.log() behind every post: at every tick fixture G10 holds, all 16 + 11 keys at
    the tolerances of the CPU test (tests/test_stream_log.py).  A stream whose pass is over keeps its last inputs."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, _lib, stream as bstream
    from boundmpc_amd.solver import _ptr
    from tests.closed_loop import fixture_mpc
    from tests.emu import emu_stream_log as elog
    passes = [(w, f, [it for it in elog.g10_passes(w) if it[0] == f]) for w in (1, 2) for f in (True, False)]
    mpcs = {w: fixture_mpc(w)[0] for w in (1, 2)}
    solver = BatchedOCPSolver(10, 4, 0.1)
    sb = bstream.StreamBatch(solver, [mpcs[w] for w, _, _ in passes])
    xphid = {w: np.array([mpcs[w].phi_max[0], 0, 0]) for w in (1, 2)}
    lib, h = solver._lib, solver._h
    assert lib.bmpc_stream_log_len(h) == bstream.log_len(10) == 884
    checked = {1: 0, 2: 0}
    for t in range(max(len(seq) for _, _, seq in passes)):
        items = [seq[min(t, len(seq) - 1)] for _, _, seq in passes]
        sb.set_robot(np.stack([it[2](xphid[w]) for it, (w, _, _) in zip(items, passes)]))
        sb.pack()
        sb.x.copy_(torch.tensor(np.stack([it[3] for it in items]))); sb.g.copy_(torch.tensor(np.stack([it[4] for it in items])))
        sb.status.copy_(torch.tensor([it[5] for it in items], dtype=torch.int32))
        sb.post(simulate=False)
        rows = sb.log()
        torch.cuda.synchronize()
        rows = rows.cpu().numpy()
        for row, it, (w, _, seq) in zip(rows, items, passes):
            if t < len(seq) and it[6]:
                elog.assert_equals_g10(row, w, it[1])
                checked[w] += 1
    assert checked == {1: elog.g10_ticks(1), 2: elog.g10_ticks(2)}
    # a missing array is an argument error, not a launch
    out = sb.log()
    args = [sb.B, _ptr(sb.path), sb.entries, _ptr(sb.state), _ptr(sb.p), _ptr(sb.traj), _ptr(out)]
    for i in (1, 3, 4, 5, 6):
        assert lib.bmpc_stream_log(h, *[None if j == i else a for j, a in enumerate(args)], None) == 1
    assert lib.bmpc_stream_log(h, sb.B, _ptr(sb.path), 4, _ptr(sb.state), _ptr(sb.p), _ptr(sb.traj), _ptr(out), None) == 1      # fewer entries than S + 1
    torch.cuda.synchronize()
    sb.close(); solver.close()


def test_device_log_equals_cpu_build_of_the_same_text():
    """bmpc_stream_log on the GPU against tests/emu's g++ build of csrc/bmpc_stream_log.inl on the same inputs (device libm vs host libm:
    round-off only; the tolerance of test_device_pack_and_post_equal_cpu_build_of_the_same_text), open loop over the ticks 0, 7, .. of
    experiment 1, and one stream of the longest horizon (N = 40: one stage per lane up to lane 39)."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload
    from oracle import c_oracle
    from tests.closed_loop import fixture_mpc
    mpc, d6 = fixture_mpc(1)
    d7 = np.load(os.path.join(G, "g7_closedloop_exp1.npz"))
    solver = BatchedOCPSolver(10, 4, 0.1)
    sb = bstream.StreamBatch(solver, [mpc])
    T, M = bstream.path_table(mpc.ref_path)
    ss = bstream.initial_state(mpc, 10); ss[bstream.SS["NENT"]] = M
    xphid = np.array([mpc.phi_max[0], 0, 0])
    for t in range(0, 155, 7):
        rb = bstream.robot_record(d7["q"][t], d7["dq"][t], d7["ddq"][t], d7["p_lie"][t], d7["v"][t], xphid, d7["jerk"][t])
        if t:                                                    # state of the stream just before tick t
            ss[bstream.SS["HASPREV"]] = 1; ss[bstream.SS["PREV"]:bstream.SS["PREV"] + 440] = d7["x"][t - 1]
            ss[bstream.SS["PHI"]], ss[bstream.SS["DPHI"]], ss[bstream.SS["DDPHI"]], ss[bstream.SS["DDDPHI"]] = (
                d7["phi_current"][t - 1], d7["dphi_current"][t - 1], d7["ddphi_current"][t - 1], d7["dddphi_current"][t - 1])
            ss[7:10], ss[10:13] = d7["pr_ref"][t - 1], d7["iw_ref"][t - 1]
            ss[0] = d7["sector"][t - 1]
        sb.state.copy_(torch.tensor(ss[None])); sb.set_robot(rb[None])
        sb.pack()
        g = c_oracle.eval_fg(d7["p"][t], d7["x"][t], 10, 4, 0.1)[1]
        sb.x.copy_(torch.tensor(d7["x"][t][None])); sb.g.copy_(torch.tensor(g[None])); sb.status.zero_()
        sb.post(simulate=False)
        rows = sb.log(); torch.cuda.synchronize()
        row = rows.cpu().numpy()[0]
        assert row[-4] == 10 and np.isfinite(row).all()
        np.testing.assert_allclose(row, _cpu_rows(sb, 10, 4, 0.1)[0], atol=1e-11, rtol=1e-11, err_msg=f"tick {t}")
    sb.close(); solver.close()
    # N = 40: a plan of random joint jerks that runs over several segment switches (the log does not ask for optimality)
    N = 40
    q0 = workload.random_q0(2, seed=7)[1]
    m40, p0fk = workload.make_mpc(q0, N=N)
    solver = BatchedOCPSolver(N, 4, 0.1)
    sb = bstream.StreamBatch(solver, [m40])
    sb.set_robot(bstream.robot_record(q0, np.zeros(7), np.zeros(7), p0fk, np.zeros(6), np.array([m40.phi_max[0], 0, 0]), np.zeros(7))[None])
    x = np.zeros((N, 44)); x[:, :7] = np.random.default_rng(0).uniform(-2.0, 2.0, (N, 7)); x[:, 7] = 0.35
    sb.pack()
    sb.x.copy_(torch.tensor(x.reshape(1, -1))); sb.g.zero_(); sb.status.zero_()
    sb.post(simulate=False)
    rows = sb.log(); torch.cuda.synchronize()
    row = rows.cpu().numpy()[0]
    assert row.shape == (88 * N + 4,) and row[-4] == N and np.isfinite(row).all()
    np.testing.assert_allclose(row, _cpu_rows(sb, N, 4, 0.1)[0], atol=1e-11, rtol=1e-11)
    sb.close(); solver.close()


@pytest.mark.parametrize("graph", [False, True])
def test_device_log_behind_the_fused_tick_and_its_graph_replay(graph):
    """Three closed-loop ticks of four workload streams (two pairs of identical streams) through sb.tick() / sb.tick_graph(): sb.log() behind
    every tick equals the CPU build of the kernel text fed with the GPU's own (path, sstate, p, traj), and the rows of identical streams
    are bit-equal."""
    import torch
    from boundmpc_amd import BatchedOCPSolver, stream as bstream, workload
    mpcs, recs = workload.make_streams(2, seed=3)
    solver = BatchedOCPSolver(10, 4, 0.1)
    sb = bstream.StreamBatch(solver, mpcs * 2)
    sb.set_robot(np.concatenate([recs, recs]))
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):      # (graph replays and the launches behind them on an explicit stream, as bench_stream.py runs them)
        for t in range(3):
            (sb.tick_graph if graph else sb.tick)(simulate=True)
            rows = sb.log()
            torch.cuda.synchronize()
            rows = rows.cpu().numpy()
            assert (rows[:, -4] == 10).all() and (rows[:, -3] == 0).all() and np.isfinite(rows).all()
            np.testing.assert_allclose(rows, _cpu_rows(sb, 10, 4, 0.1), atol=1e-11, rtol=1e-11, err_msg=f"tick {t}")
            assert np.array_equal(rows[0], rows[2]) and np.array_equal(rows[1], rows[3])
    torch.cuda.synchronize()
    sb.close(); solver.close()
