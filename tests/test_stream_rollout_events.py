"""Events inside a rollout -- plant disturbances and one scheduled re-plan per stream with the measured state spliced in on the device -- as device code
compiled for the CPU (csrc/bmpc_rollout_kernel.inl with EV, csrc/bmpc_stream_events.inl; tests/emu/bmpc_emu_rollout.cpp, bmpc_emu_stream_update.cpp): without events the
rollout's own bits; with events the bits of the per-tick loop {fused tick's text, disturb text, splice + update text at the scheduled tick}; the splice
and the disturbance against their numpy mirrors (stream.splice_record, stream.disturb_robot) and NodeLoop.update; the rescue of a stream whose plan
ran out, the second leg behind a reached goal, and the argument errors.  B = 3 streams of emu_rollout.small_stream, T = 6."""
import numpy as np
import pytest

from boundmpc_amd import stream as bstream, workload
from boundmpc_amd.bound_mpc import integrate_joint
from boundmpc_amd.robot_model import RobotModel
from tests.emu import emu_rollout as er, emu_stream_update as eup

SS, RB, RP, RV, ROLL = bstream.SS, bstream.RB, bstream.RP, bstream.RV, bstream.ROLL
H, T = er.H, 6
ATOL = 1e-11                     # tests/test_stream_update.py's; the header words a and jerk hold it too (measured: profiles/stream_splice.txt)


_copy = er.copy_arrays


def _against_the_loop(N, S, A0, Tab, recs, ticks, replan_tick, disturb, what, update_flags=3, goal_tol=0.0, **kw):
    """the events text on copies of (A0, Tab, recs) against the per-tick loop, stream by stream, on other copies: every tick array, the path table, the
    record buffer, hist, traj_hist, ticks_run and replan_info, bit for bit.  -> (result, arrays, tables, records) of the events text"""
    A, Tb, R = _copy(A0), Tab.copy(), recs.copy()
    r = er.rollout(N, S, H, Tb, A, ticks, entry=1, replan=R, replan_tick=replan_tick, update_flags=update_flags, disturb=disturb, goal_tol=goal_tol, **kw)
    for b in range(Tab.shape[0]):
        Ab, Tl, Rl = er.unstack(A0, b), Tab[b].copy(), recs[b].copy()
        loop = er.contract_loop(N, S, H, Tl, Ab, ticks, replan=Rl, replan_tick=int(replan_tick[b]), update_flags=update_flags,
                                disturb=None if disturb is None else disturb[:, b], goal_tol=goal_tol, **kw)
        rows, trajs, run, info = loop["hist"], loop["traj_hist"], loop["ticks_run"], loop["replan_info"]
        er.assert_arrays_equal(Ab, er.unstack(A, b), f"{what}, stream {b}")
        assert np.array_equal(Tl, Tb[b], equal_nan=True) and np.array_equal(Rl, R[b], equal_nan=True), f"{what}, stream {b}: table / record"
        assert np.array_equal(rows, r["hist"][:, b], equal_nan=True) and np.array_equal(trajs, r["traj_hist"][:, b], equal_nan=True), f"{what}, stream {b}: history"
        assert (run, info) == (r["ticks_run"][b], r["replan_info"][b]), f"{what}, stream {b}: ticks_run / replan_info"
    return r, A, Tb, R


@pytest.mark.parametrize("N,S", [(2, 2), (1, 2)])
def test_without_events_the_events_text_equals_the_rollout_text(N, S):
    """every event pointer NULL: all tick arrays, hist, traj_hist and ticks_run of the rollout's own CPU build, bit for bit; the table stays"""
    _, A0, Tab, _ = er.small_batch(N, S)
    A, Tb = _copy(A0), Tab.copy()
    r = er.rollout(N, S, H, Tb, A, T, entry=1)
    plain = _copy(A0)
    r0 = er.rollout(N, S, H, Tab.copy(), plain, T, entry=1, level=0)      # (the instantiation without the event code, B = 3 on one workgroup)
    assert np.array_equal(Tb, Tab) and r["replan_info"].tolist() == [-1] * 3
    for b in range(3):
        Ab = er.unstack(A0, b)
        want = er.rollout(N, S, H, Tab[b], Ab, T, warm_dual=True)
        er.assert_arrays_equal(Ab, er.unstack(A, b), f"stream {b}")
        er.assert_arrays_equal(Ab, er.unstack(plain, b), f"stream {b}, EV = false")
        assert np.array_equal(r["hist"][:, b], want["hist"]) and np.array_equal(r["traj_hist"][:, b], want["traj_hist"]) and r["ticks_run"][b] == want["ticks_run"] == T
        assert np.array_equal(r0["hist"][:, b], want["hist"]) and r0["ticks_run"][b] == T


@pytest.mark.parametrize("N,S", [(2, 2), (1, 2)])
def test_events_equal_the_per_tick_loop_bit_for_bit(N, S):
    """Re-plans (splice, set_goal) behind tick 2 of stream 0 and behind the last tick of stream 2, none for stream 1 (replan_tick -1); disturbances on
    ticks 1 and 4.  The new path -- a leg back over the stream's own via points from the spliced pose -- is a good input: every tick behind the re-plan
    converges and its plan is applied."""
    _, A0, Tab, recs = er.small_batch(N, S)
    tick_of = np.array([2, -1, T - 1])
    dist = er.disturbances(T, 3, on=(1, 4))
    r, A, Tb, R = _against_the_loop(N, S, A0, Tab, recs, T, tick_of, dist, f"N {N} S {S}")
    assert r["ticks_run"].tolist() == [T] * 3 and r["replan_info"].tolist() == [0, -1, 0]
    assert R[:, RP["FLAG"]].tolist() == [0.0, 1.0, 0.0] and np.array_equal(R[1], recs[1]) and np.array_equal(Tb[1], Tab[1])
    assert (r["hist"][:, :, ROLL["STATUS"]] == 0).all() and (r["hist"][:, :, ROLL["SUCCESS"]] == 1).all() and (r["hist"][:, :, ROLL["ERRCNT"]] == 0).all()
    # the re-plan took: a new table and phi_max, the goal follows, phi starts again on the new first segment and the stream moves on
    for b in (0, 2):
        assert not np.array_equal(Tb[b], Tab[b]) and A["ss"][b, SS["PHIMAX"]] != A0["ss"][b, SS["PHIMAX"]] and A["ss"][b, bstream.ss_updated(N)] == 1.0
        assert A["rb"][b, RB["XPHID"]] == A["ss"][b, SS["PHIMAX"]]
    phi = r["hist"][:, 0, ROLL["PHI"]]
    assert phi[3] < phi[2] and (np.diff(phi[3:]) > 0).all()
    # the spliced words stay in the record: the pose behind tick 2, which hist shows (no disturbance on that tick)
    row = r["hist"][2, 0]
    assert np.array_equal(R[0, RP["P0"]:RP["P0"] + 3], row[RB["P"]:RB["P"] + 3]) and np.array_equal(R[0, RP["V"]:RP["V"] + 3], row[RB["V"]:RB["V"] + 3])
    # hist shows the UNDISTURBED plant behind a tick: without the disturbances ticks 0 and 1 have the same rows, tick 2 differs
    r1 = er.rollout(N, S, H, Tab.copy(), _copy(A0), T, entry=1, replan=recs.copy(), replan_tick=tick_of)
    assert np.array_equal(r1["hist"][:2], r["hist"][:2]) and not np.array_equal(r1["hist"][2], r["hist"][2])
    # in any lane order of the solver's phases
    for order in (1, 2):
        C, Tc, Rc = _copy(A0), Tab.copy(), recs.copy()
        rc = er.rollout(N, S, H, Tc, C, T, entry=1, replan=Rc, replan_tick=tick_of, disturb=dist, lane_order=order)
        assert np.array_equal(rc["hist"], r["hist"]) and np.array_equal(C["ss"], A["ss"]) and np.array_equal(Tc, Tb)


def _random_robot(rng, which):
    """a robot record in motion: joint state with non-zero dq, ddq and jerk, its pose and Cartesian velocity"""
    model = RobotModel()
    q = workload.random_q0(which + 1, seed=11)[which]
    dq, ddq, u = rng.normal(size=7) * 0.3, rng.normal(size=7) * 0.8, rng.normal(size=7) * 3.0
    p, J, _ = model.forward_kinematics(q, dq)
    return bstream.robot_record(q, dq, ddq, p, J @ dq, np.array([3.0, 0.0, 0.0]), u)


_SPLICE_WORST = {}


@pytest.mark.parametrize("case", range(6))
def test_splice_equals_the_numpy_mirror(case):
    """The CPU build's stream_splice against stream.splice_record on a record of a random path and a robot record in motion; then the update text on the
    spliced record against apply_update fed the mirror's numbers (table, state).  Cases 0..3 walk the poor-bounds rule over both sides of both of its
    conditions (the rule on), cases 4, 5 have the rule off where its condition holds / a (1, 2) shape."""
    rng = np.random.default_rng(400 + case)
    N, S = ((10, 4), (2, 2), (10, 4), (2, 2), (10, 4), (1, 2))[case]
    poor = case < 4
    path = eup.random_path(rng, 3 + case % 3, nb=1 + case % 2)
    entries = len(path["pos_points"]) + S - 1 + case % 2
    rb = _random_robot(rng, case)
    v2_neg, y_opposed = ((True, True), (True, False), (False, True), (False, False), (True, True), (True, True))[case]
    rb[RB["V"] + 2] = -abs(rb[RB["V"] + 2]) - 0.01 if v2_neg else abs(rb[RB["V"] + 2]) + 0.01
    path["pos_points"][1][1] = (-1.0 if y_opposed else 1.0) * np.sign(rb[RB["P"] + 1]) * (abs(path["pos_points"][1][1]) + 0.05)
    rec0 = bstream.replan_record(S, entries, *eup.args_of(path))
    got, want = eup.stream_splice(H, S, rec0, rb, poor_bounds=poor), bstream.splice_record(rec0, rb, H, S, poor_bounds=poor)
    # what the splice writes, and nothing else
    words = np.r_[RP["P0"]:RP["P0"] + 12, RP["HEAD"] + RV["P"]:RP["HEAD"] + RV["R"] + 9]
    rest = np.setdiff1d(np.arange(rec0.shape[0]), words)
    assert np.array_equal(got[rest], rec0[rest]) and np.array_equal(want[rest], rec0[rest]) and got[RP["FLAG"]] == 1.0
    aj = np.r_[RP["A"]:RP["A"] + 6]
    dev_aj, dev = float(np.abs(got[aj] - want[aj]).max()), float(np.abs(got[np.setdiff1d(words, aj)] - want[np.setdiff1d(words, aj)]).max())
    _SPLICE_WORST[case] = (dev, dev_aj)
    print(f"case {case}: N {N} S {S}: splice, CPU build - numpy mirror: {dev:.3e}; header a, jerk: {dev_aj:.3e} (|a| {np.abs(want[RP['A']:RP['A'] + 3]).max():.2f}, "
          f"|jerk| {np.abs(want[RP['JERK']:RP['JERK'] + 3]).max():.2f}); worst so far {max(v[0] for v in _SPLICE_WORST.values()):.3e} / {max(v[1] for v in _SPLICE_WORST.values()):.3e}")
    assert dev <= ATOL and dev_aj <= ATOL
    lowered = poor and v2_neg and y_opposed
    z = rb[RB["P"] + 2] + 0.5 * H * rb[RB["V"] + 2] - (0.05 if lowered else 0.0)
    assert abs(got[RP["HEAD"] + RV["P"] + 2] - z) < 1e-15 and np.array_equal(got[RP["P0"]:RP["P0"] + 3], rb[RB["P"]:RB["P"] + 3])
    # ... and through the update: table and state against apply_update on the mirror's numbers
    ss0 = eup.random_state(rng, N, has_prev=True)
    info, rec1, Tn, ss, rb1 = eup.stream_update_flags(N, S, H, rec0, np.random.default_rng(9).normal(size=(entries, bstream.PT["LEN"])), ss0, rb, 3 | (4 if poor else 0))
    assert info == 0 and rec1[RP["FLAG"]] == 0.0 and np.array_equal(rec1[1:], got[1:])      # the spliced words stay, only the flag is cleared
    ss_ref = ss0.copy()
    T_ref, M = bstream.apply_update(ss_ref, N, S, *er.args_of_record(want, S), entries=entries)
    eup.assert_close(Tn, ss, T_ref, ss_ref, ATOL, f"case {case}: update behind the splice")
    assert rb1[RB["XPHID"]] == ss[SS["PHIMAX"]] and np.array_equal(np.delete(rb1, np.r_[RB["XPHID"]:RB["XPHID"] + 3]), np.delete(rb, np.r_[RB["XPHID"]:RB["XPHID"] + 3]))


def test_splice_leaves_a_lowered_flag_and_an_invalid_record_alone():
    rng = np.random.default_rng(21)
    N, S, entries = 2, 2, 6
    rec0, rb = bstream.replan_record(S, entries, *eup.args_of(eup.random_path(rng, 4))), _random_robot(rng, 0)
    Tg, ss0 = rng.normal(size=(entries, bstream.PT["LEN"])), eup.random_state(rng, N)
    low = rec0.copy(); low[RP["FLAG"]] = 0.0
    assert np.array_equal(eup.stream_splice(H, S, low, rb), low) and np.array_equal(bstream.splice_record(low, rb, H, S), low)
    info, rec1, T1, ss1, rb1 = eup.stream_update_flags(N, S, H, low, Tg, ss0, rb, 7)
    assert info == 0 and np.array_equal(rec1, low) and np.array_equal(T1, Tg) and np.array_equal(ss1, ss0) and np.array_equal(rb1, rb)
    for n, nb in ((1, 1), (6, 2), (4, 0), (4, 5), (np.nan, 1), (4, np.inf)):      # n_max = 5
        bad = rec0.copy(); bad[RP["N"]], bad[RP["NB"]] = n, nb
        assert np.array_equal(eup.stream_splice(H, S, bad, rb, poor_bounds=True), bad, equal_nan=True) and np.array_equal(bstream.splice_record(bad, rb, H, S, True), bad, equal_nan=True)
        info, rec1, T1, ss1, rb1 = eup.stream_update_flags(N, S, H, bad, Tg, ss0, rb, 3)
        assert info == 1 and rec1[RP["FLAG"]] == 0.0 and np.array_equal(rec1[1:], bad[1:], equal_nan=True) and np.array_equal(T1, Tg) and np.array_equal(ss1, ss0)
    # the flags bmpc_stream_update refuses: an unknown bit, poor bounds without the splice, the splice without robot records
    for flags, robot in ((8, rb), (4, rb), (5, rb), (2, None), (3, None)):
        assert eup.stream_update_flags(N, S, H, rec0, Tg, ss0, robot, flags)[0] == -2, flags
    # flags 0 and 1 are the update text alone
    for flags in (0, 1):
        a, b = eup.stream_update_flags(N, S, H, rec0, Tg, ss0, rb, flags), eup.stream_update(N, S, rec0, Tg, ss0, rb, set_goal=bool(flags))
        assert a[0] == b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_disturbance_equals_the_numpy_mirror():
    rng = np.random.default_rng(31)
    rb = _random_robot(rng, 1)
    assert np.array_equal(eup.stream_disturb(rb, np.zeros(21)), rb) and np.array_equal(bstream.disturb_robot(rb, np.zeros(21)), rb)
    assert np.array_equal(eup.stream_disturb(rb, np.full(21, np.nan)), rb) and np.array_equal(eup.stream_disturb(rb, -np.zeros(21)), rb)
    d = rng.normal(size=21) * 0.05
    got, want = eup.stream_disturb(rb, d), bstream.disturb_robot(rb, d)
    assert np.array_equal(got[:21], rb[:21] + d) and np.array_equal(got[RB["XPHID"]:], rb[RB["XPHID"]:])
    np.testing.assert_allclose(got, want, atol=ATOL, rtol=0)
    assert np.abs(got[RB["P"]:RB["P"] + 6] - rb[RB["P"]:RB["P"] + 6]).max() > 1e-3
    d2 = d.copy(); d2[[0, 9, 20]] = [np.nan, np.inf, -np.inf]      # non-finite entries count as 0
    d3 = d.copy(); d3[[0, 9, 20]] = 0.0
    assert np.array_equal(eup.stream_disturb(rb, d2), eup.stream_disturb(rb, d3)) and np.array_equal(bstream.disturb_robot(rb, d2), bstream.disturb_robot(rb, d3))


def test_node_loop_update_passes_what_the_splice_writes_but_for_the_jerk():
    """NodeLoop.update (bound_mpc_node.py:121-165) in the state the node's own plant step left: the arguments it hands to BoundMPC.update are the words
    the splice mirror writes into a record of the same path from the robot record of that state -- except the jerk, where the node takes ddJ at the state
    before the step and J ddq in the place of J u."""
    from boundmpc_amd.node_loop import NodeLoop
    rng = np.random.default_rng(41)
    q0 = workload.random_q0(1, seed=5)[0]
    model = RobotModel()
    p0fk = model.fk(q0)
    path = workload.experiment1_path(p0fk)
    seq = ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min", "e_p_max", "e_r_max")
    loop = NodeLoop(*[path[k] for k in seq], p0=p0fk, q0=q0, params=workload.Params(n=2, nr_segs=2), solver=workload._NoSolver())
    # one plant step of the node from a state in motion (step(), :346-360): jerk matrix [current, u0, u1]
    q, dq, ddq, jm = q0 + rng.normal(size=7) * 0.05, rng.normal(size=7) * 0.3, rng.normal(size=7) * 0.8, rng.normal(size=(7, 3)) * 3.0
    loop.q, loop.dq, loop.ddq, loop.p_lie, loop.v, loop.a, loop.j_cart = integrate_joint(model, jm, q, dq, ddq, loop.mpc.dt)
    loop.jerk = jm[:, 1].copy()
    loop.v[2] = -abs(loop.v[2])                                  # (scenario 0 on its lowering side)
    new = workload.experiment2_path(p0fk)
    new["pos_points"][1][1] = -np.sign(loop.p_lie[1]) * 0.3
    seen = {}
    loop.mpc.update = lambda *a, **k: seen.update(a=a, k=k)
    loop.mpc.phi_max = np.array([1.25])
    p_via, r_via = loop.update(*[new[k] for k in seq])
    a = seen["a"]
    rb = bstream.robot_record(loop.q, loop.dq, loop.ddq, loop.p_lie, loop.v, loop.x_phi_d, loop.jerk)
    rec = bstream.replan_record(2, 6, *[new[k] for k in seq], np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), np.zeros(6), workload.default_weights())
    spl = bstream.splice_record(rec, rb, loop.mpc.dt, 2, poor_bounds=True)
    via0 = spl[RP["HEAD"]:RP["HEAD"] + RV["LEN"]]
    assert np.array_equal(a[0][0], via0[RV["P"]:RV["P"] + 3]) and np.allclose(a[1][0].reshape(9), via0[RV["R"]:RV["R"] + 9], atol=1e-15, rtol=0)
    assert abs(a[0][0][2] - (loop.p_lie[2] + 0.5 * 0.1 * loop.v[2] - 0.05)) < 1e-15 and all(np.array_equal(x, y) for x, y in zip(a[0][1:], new["pos_points"][1:]))
    assert np.array_equal(seen["k"]["p0"][:3], spl[RP["P0"]:RP["P0"] + 3]) and np.array_equal(a[11], loop.p_lie) and np.array_equal(a[12][:3], spl[RP["V"]:RP["V"] + 3])
    np.testing.assert_allclose(a[13][:3], spl[RP["A"]:RP["A"] + 3], atol=1e-12, rtol=0)      # the node's a is this a
    dj = a[14][:3] - spl[RP["JERK"]:RP["JERK"] + 3]
    print(f"jerk: node's j_cart {a[14][:3]}, consistent derivative {spl[RP['JERK']:RP['JERK'] + 3]}, difference {dj} (largest {np.abs(dj).max():.3e})")
    assert np.abs(dj).max() > 1e-3                                # ... and the jerk is another quantity
    assert np.array_equal(loop.x_phi_d, [1.25, 0.0, 0.0]) and np.array_equal(loop.q0, loop.q) and np.array_equal(loop.p0, loop.p_lie)
    assert loop.update(*[new[k] for k in seq], update=False) is None      # msg.update false: the trajectory is kept, nothing else happens


def test_a_replan_behind_the_post_that_exhausted_the_plan_rescues_the_stream():
    """(2, 2), tick 0 solved out, then one iteration a tick without the real-time acceptance, on plants that a push has carried 16 cm off their paths
    (tube half width at the start: 1 cm; two stages cannot bring them back): every tick then fails.  (Without the push the one-iteration ticks of these
    streams keep a summed violation of 0 and never fail, like the two-iteration ticks of tests/test_stream_rollout.py.)  From error count 0 a stream
    runs 2 ticks and is lost; re-planned behind tick 1 (error count N -> N - 1) it runs a third.  A stream lost on entry never consumes a record
    scheduled for tick 0.  Solved to tolerance, the spliced re-plan is a rescue in earnest: the new path starts where the plant is, and the stream runs on."""
    N, S = 2, 2
    _, A0, Tab, recs = er.small_batch(N, S)
    push = np.zeros(21); push[:4] = [0.1, -0.1, 0.1, 0.1]
    for b in range(3):
        Ab = er.unstack(A0, b)
        er.tick(N, S, H, Tab[b], Ab, max_iter=100, warm_dual=True)
        Ab["rb"] = eup.stream_disturb(Ab["rb"], push)
        for k in A0:
            A0[k][b] = Ab[k]
    assert (A0["status"] == 0).all() and (A0["ss"][:, SS["ERRCNT"]] == 0).all() and (A0["ss"][:, SS["HASPREV"]] == 1).all()
    lost = _copy(A0); lost["ss"][2, SS["ERRCNT"]] = N              # stream 2: lost on entry
    tick_of = np.array([1, -1, 0])
    r, A, Tb, R = _against_the_loop(N, S, lost, Tab, recs, T, tick_of, None, "rescue", max_iter=1)
    assert r["ticks_run"].tolist() == [3, 2, 0] and r["replan_info"].tolist() == [0, -1, -1] and R[:, RP["FLAG"]].tolist() == [0.0, 1.0, 1.0]
    h = r["hist"]
    assert h[:3, 0, ROLL["ERRCNT"]].tolist() == [1, 2, 2] and h[:2, 1, ROLL["ERRCNT"]].tolist() == [1, 2]
    assert (h[:3, 0, ROLL["SUCCESS"]] == 0).all() and (h[:2, 1, ROLL["SUCCESS"]] == 0).all() and (h[:3, 0, ROLL["STATUS"]] == 1).all() and (h[:3, 0, ROLL["GVIOL"]] > 1e-4).all()
    assert np.isfinite(h[:3, 0]).all() and np.isnan(h[3:, 0]).all() and np.isnan(h[2:, 1]).all() and np.isnan(h[:, 2]).all() and np.isnan(r["traj_hist"][3:, 0]).all()
    assert A["status"].ravel().tolist() == [3, 3, 3] and np.array_equal(Tb[2], Tab[2]) and np.array_equal(R[2], recs[2])
    keep = er.unstack(lost, 2); keep["status"][0], keep["iters"][0], keep["kkt"][0] = 3, 0, 0.0
    er.assert_arrays_equal(keep, er.unstack(A, 2), "lost on entry: nothing but the three words of a skipped stream")
    full, _, _, _ = _against_the_loop(N, S, A0, Tab, recs, T, np.array([1, -1, 1]), None, "rescue, solved to tolerance")
    assert full["ticks_run"].tolist() == [T, 2, T] and (full["hist"][2:, [0, 2], ROLL["SUCCESS"]] == 1).all() and (full["hist"][2:, [0, 2], ROLL["ERRCNT"]] == 0).all()


def test_a_replan_behind_the_tick_that_reaches_the_goal_starts_a_second_leg():
    """goal_tol from the stream's own phi trace, reached behind tick tg - 1 (tg ticks run): with a re-plan scheduled behind that tick the stream does not
    stop there -- the goal test sees the new phi_max -- and runs every tick, on the new path, as the per-tick loop under the same rule does.  (The goal
    tolerance of this construction is nearly the whole path, so the second leg is 0.1 m longer than the first: its goal stays out of reach for T ticks.)"""
    N, S = 2, 2
    _, A0, Tab, recs = er.small_batch(N, S, B=1, detour=0.05)
    free = er.rollout(N, S, H, Tab.copy(), _copy(A0), T, entry=1)
    gap = A0["ss"][0, SS["PHIMAX"]] - free["hist"][:, 0, ROLL["PHI"]]
    goal_tol = float(gap[1])
    stop = er.rollout(N, S, H, Tab.copy(), _copy(A0), T, entry=1, goal_tol=goal_tol)
    tg = int(stop["ticks_run"][0])
    assert tg == 2 < T and np.isnan(stop["hist"][tg:]).all()
    r, A, Tb, R = _against_the_loop(N, S, A0, Tab, recs, T, np.array([tg - 1]), None, "second leg", goal_tol=goal_tol)
    assert r["ticks_run"].tolist() == [T] and r["replan_info"].tolist() == [0] and np.isfinite(r["hist"]).all()
    ss_ref = A0["ss"][0].copy()
    want = bstream.splice_record(recs[0], r["hist"][tg - 1, 0, :RB["LEN"]], H, S)
    T_ref, _ = bstream.apply_update(ss_ref, N, S, *er.args_of_record(want, S), entries=Tab.shape[1])
    assert abs(A["ss"][0, SS["PHIMAX"]] - ss_ref[SS["PHIMAX"]]) < ATOL and A["rb"][0, RB["XPHID"]] == A["ss"][0, SS["PHIMAX"]] != A0["ss"][0, SS["PHIMAX"]]
    assert np.abs(Tb[0] - T_ref).max() < ATOL
    late = _against_the_loop(N, S, A0, Tab, recs, T, np.array([tg]), None, "a re-plan one tick late", goal_tol=goal_tol)[0]      # stops win over events
    assert late["ticks_run"].tolist() == [tg] and late["replan_info"].tolist() == [-1]


def test_argument_errors_of_the_entry():
    """what the C ABI refuses beside the rollout's own errors: a record buffer without its ticks, the update flags bmpc_stream_update refuses"""
    N, S = 2, 2
    _, A0, Tab, recs = er.small_batch(N, S)
    ok = dict(replan=recs, replan_tick=[1, 1, 1], update_flags=3)
    bad = [dict(ok, replan_tick=None), dict(ok, update_flags=8), dict(ok, update_flags=4), dict(ok, update_flags=5), dict(ok, update_flags=-1), dict(update_flags=16),
           dict(ok, ticks=0), dict(ok, simulate=False), dict(ok, goal_tol=-1.0), dict(ok, goal_tol=np.nan)]
    for kw in bad:
        A, Tb = _copy(A0), Tab.copy()
        kw = dict(kw); kw["replan"] = None if kw.get("replan") is None else recs.copy()
        assert er.rollout(N, S, H, Tb, A, kw.pop("ticks", 2), entry=1, want_rc=True, **kw) == 1, kw
        for b in range(3):
            er.assert_arrays_equal(er.unstack(A0, b), er.unstack(A, b), "nothing runs")
        assert np.array_equal(Tb, Tab) and (kw["replan"] is None or np.array_equal(kw["replan"], recs))
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=1, update_flags=2, want_rc=True) == 0      # the splice bit without records: allowed, ignored
    assert er.rollout(N, S, H, Tab.copy(), _copy(A0), 2, entry=1, want_rc=True, **dict(ok, replan=recs.copy())) == 0


def test_lengths_and_the_python_surface():
    assert bstream.DIST_LEN == 21 and eup.lib().bmpc_emu_stream_disturb_len() == 21
    import inspect
    for fn, names in ((bstream.StreamBatch.update_device, ("splice", "poor_bounds")), (bstream.StreamBatch.rollout, ("replan", "replan_tick", "splice", "poor_bounds", "set_goal", "disturb")),
                      (bstream.StreamBatch.disturb, ("d", "stream"))):
        assert set(names) <= set(inspect.signature(fn).parameters)
    with pytest.raises(ValueError, match="poor_bounds"):
        bstream.StreamBatch._update_flags(True, False, True)
    assert bstream.StreamBatch._update_flags(True, True, True) == 7 and bstream.StreamBatch._update_flags(False, True, False) == 2
