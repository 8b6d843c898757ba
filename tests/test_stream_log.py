"""The logging records of BoundMPC.step() on the stream functions (csrc/bmpc_stream_log.inl compiled for the CPU, tests/emu): ref_data / err_data
per stage of the plan a tick left behind, against
  (i) the reference's own dictionaries on the recorded experiments (fixture G10, tests/golden/make_g10.py), the forced solver failure included,
 (ii) the host mirror BoundMPC._logging_data on a synthetic closed loop with failures,
(iii) the contract of the row: no plan -> n_valid 0 and NaN, non-finite inputs -> non-finite records, the smallest and largest index ranges."""
import numpy as np
import pytest

from boundmpc_amd import stream as bstream, workload
from boundmpc_amd.bound_mpc import integrate_joint
from boundmpc_amd.robot_model import RobotModel
from tests.closed_loop import Oracle, cpu_mirror_loop, fixture_mpc, stream_arrays
from tests.emu import emu, emu_stream_log as elog


@pytest.mark.parametrize("which", [1, 2])
def test_log_of_the_kernel_text_equals_the_references_dictionaries_g10(which):
    """Open loop over the recorded ticks (the robot state and the solution of every tick from fixture G7, as
    test_stream_pack_is_exact_given_the_reference_state): pack -> post -> log, every tick; at every tick fixture G10 holds all 16 + 11 keys
    equal the reference's.  Tolerances: ten times the host mirror's against the same fixture -- the kernel starts from the device pack's p,
    itself held to 2e-11 against the reference's."""
    checked = 0
    for with_failure, t, rec, x, g, status, check in elog.g10_passes(which):
        if t == 0:
            mpc, _ = fixture_mpc(which, Oracle())
            T, ss = stream_arrays(mpc, 10)
            xphid = np.array([mpc.phi_max[0], 0, 0])
        rb = rec(xphid)
        p, _ = emu.stream_pack(10, 4, T, ss, rb)
        traj = emu.stream_post(10, 4, 0.1, T, ss, rb.copy(), x, g, status, simulate=False)
        row = elog.stream_log(10, 4, 0.1, T, ss, p, traj)
        assert int(row[-4]) == 10 - int(row[-3]) == int(traj[-4]) and row[-3] == ss[bstream.SS["ERRCNT"]]
        if check:
            elog.assert_equals_g10(row, which, t)
            checked += 1
    assert checked == elog.g10_ticks(which)


def _same_rotations(a, b, tol):
    from scipy.spatial.transform import Rotation as R
    np.testing.assert_allclose(R.from_rotvec(a).as_matrix(), R.from_rotvec(b).as_matrix(), atol=tol)


def _assert_equals_mirror(row, ref, err, N, tol, dtol, what):
    """a log row against the host mirror's dictionaries; ref p[3:] as rotations (at angle pi the sign of a rotation vector is round-off)"""
    got_ref, got_err = bstream.unpack_log(row, N)
    n = len(ref["p"])
    assert int(row[-4]) == n == len(got_ref["p"]) == len(got_err["e_p"])
    assert np.isnan(row[n * bstream.LOG_STAGE:N * bstream.LOG_STAGE]).all() and np.isfinite(row[:n * bstream.LOG_STAGE]).all()
    for k in elog.REF_KEYS:
        got, want = np.array(got_ref[k]), np.array(ref[k]).reshape(n, -1)
        assert got.shape == want.shape, k
        if k == "p":
            _same_rotations(got[:, 3:], want[:, 3:], tol)
            got, want = got[:, :3], want[:, :3]
        np.testing.assert_allclose(got, want, atol=tol, rtol=0, err_msg=f"{what} ref {k}")
    for k in elog.ERR_KEYS:
        got, want = np.array(got_err[k]), np.array(err[k]).reshape(n, -1)
        assert got.shape == want.shape, k
        np.testing.assert_allclose(got, want, atol=dtol if k.startswith("de_") else tol, rtol=0, err_msg=f"{what} err {k}")


def test_log_matches_host_mirror_with_failures():
    """The synthetic stream of test_stream_matches_host_mirror_with_failures (solver failing at ticks 3, 4 and 9), the host mirror logging
    (real_time off): n_valid / error_count of every tick's log equal the mirror's, every key agrees within that test's tolerances (two
    independently rounded closed loops), stages at or beyond n_valid are NaN."""
    q0 = workload.random_q0(3, seed=5)[2]
    fails = (3, 4, 9)
    mpc, p0fk = workload.make_mpc(q0, solver=Oracle(fails))
    mpc.log = True                                    # params.real_time = False (BoundMPC.py:47)
    ref_mpc, _ = workload.make_mpc(q0, solver=Oracle())
    T, _ = stream_arrays(ref_mpc, 10)
    rm = RobotModel()
    q, dq, ddq, jerk, v = q0.copy(), np.zeros(7), np.zeros(7), np.zeros(7), np.zeros(6)
    x_phi_d = np.array([mpc.phi_max[0], 0, 0])
    seen = []
    for c in cpu_mirror_loop(ref_mpc, bstream.robot_record(q, dq, ddq, p0fk, v, x_phi_d, jerk), 14, solve=Oracle(fails).solve):
        t = c["t"]
        row = elog.stream_log(10, 4, 0.1, T, c["ss"], c["p"], c["traj"])
        p_lie = rm.forward_kinematics(q, dq)[0]
        traj, ref, err, _, _ = mpc.step(q, dq, ddq, p_lie, v, x_phi_d, jerk)
        assert int(row[-3]) == mpc.error_count and int(row[-4]) == 10 - mpc.error_count
        seen.append(mpc.error_count)
        _assert_equals_mirror(row, ref, err, 10, 2e-6, 2e-5, f"tick {t}")
        jm = np.concatenate((jerk[:, None], traj["dddq"][:, :2]), axis=1)
        q, dq, ddq, p_lie, v = integrate_joint(rm, jm, q, dq, ddq, mpc.dt)[:5]
        jerk = traj["dddq"][:, 0].copy()
    assert seen[3] == 1 and seen[4] == 2 and seen[5] == 0 and seen[9] == 1


class _Answer:
    """nlpsol-shaped stub answering with a given plan, feasible by declaration"""

    def __init__(self, x):
        self.x = np.asarray(x, dtype=float)

    def generate_dependencies(self, *a, **k):
        pass

    def __call__(self, x0=None, lbx=None, ubx=None, lbg=None, ubg=None, p=None):
        return {"x": self.x.reshape(-1, 1), "g": np.zeros((len(lbg), 1)), "f": 0.0, "lam_x": 0 * self.x, "lam_g": np.zeros(len(lbg))}

    def stats(self):
        return {"iter_count": 1, "success": True, "return_status": "stub"}


def _one_tick(N, S, jerk_phi, seed=0):
    """One tick of a stream at rest whose `solver` answers with a plan of random joint jerks and the path jerk `jerk_phi` (the log does not
    ask for optimality: both sides re-integrate the plan from its jerks) -> (mirror, its ref, err, and the stream's T, ss, p, traj)."""
    dt = 0.1
    q0 = workload.random_q0(2, seed=7)[1]
    rng = np.random.default_rng(seed)
    x = np.zeros((N, 44))
    x[:, :7] = rng.uniform(-2.0, 2.0, (N, 7)); x[:, 7] = jerk_phi
    mpc, p0fk = workload.make_mpc(q0, N=N, S=S, dt=dt, solver=_Answer(x.ravel()))
    mpc.log = True
    fresh, _ = workload.make_mpc(q0, N=N, S=S, dt=dt)
    T, ss = stream_arrays(fresh, N)
    z7, xphid = np.zeros(7), np.array([mpc.phi_max[0], 0, 0])
    rb = bstream.robot_record(q0, z7, z7, p0fk, np.zeros(6), xphid, z7)
    _, ref, err, _, _ = mpc.step(q0, z7, z7, p0fk, np.zeros(6), xphid, z7)
    p, _ = emu.stream_pack(N, S, T, ss, rb)
    traj = emu.stream_post(N, S, dt, T, ss, rb.copy(), x.ravel(), np.zeros(43 * N), 0, simulate=False)
    return mpc, ref, err, T, ss, p, traj


# (N, S, jerk of the path parameter): the smallest and the largest stage range, the smallest and the largest window; the long plan runs over
# several segment switches (re-anchored rotation reference, every segment row), the two-segment window stays short of its second switch
@pytest.mark.parametrize("N,S,jerk_phi", [(1, 4, 3.0), (40, 4, 0.35), (10, 2, 1.0), (10, 6, 6.0)])
def test_log_index_ranges_against_host_mirror(N, S, jerk_phi):
    """Same inputs on both sides, so the host mirror's own tolerances against the reference hold times ten (see the G10 test)."""
    mpc, ref, err, T, ss, p, traj = _one_tick(N, S, jerk_phi)
    row = elog.stream_log(N, S, 0.1, T, ss, p, traj)
    assert row.shape == (88 * N + 4,) and int(row[-4]) == N and int(row[-3]) == 0
    _assert_equals_mirror(row, ref, err, N, 1e-10, 1e-9, f"N={N} S={S}")
    if N == 40:      # the plan does cross segment switches: the segment rows and the re-anchoring are exercised
        sw = p[bstream._poff(S)["sw"]:][:S + 1]
        phi = bstream.unpack_traj(traj, N)[0]["phi"]
        assert phi[0] < sw[1] < phi[-1] and phi[-1] > sw[2]


def test_log_of_a_stream_without_a_plan_is_nan():
    """error_count >= N (step() returns Nones; the fused tick skips the stream and leaves its arrays stale): n_valid = 0, all-NaN body."""
    _, _, _, T, ss, p, traj = _one_tick(10, 4, 1.0)
    assert np.isfinite(elog.stream_log(10, 4, 0.1, T, ss, p, traj)[:880]).all()
    for ec in (10, 11, np.nan):
        s2 = ss.copy(); s2[bstream.SS["ERRCNT"]] = ec
        row = elog.stream_log(10, 4, 0.1, T, s2, p, traj)
        assert row[-4] == 0 and np.isnan(row[:880]).all() and np.isfinite(row[880:]).all()
        assert bstream.unpack_log(row, 10) == (None, None)


def test_log_of_non_finite_inputs_is_non_finite_and_returns():
    """A NaN planted in traj (a path parameter, a pose entry), in the state or in p: the function returns, the records that depend on it
    are non-finite, the counts stay."""
    _, _, _, T, ss, p, traj = _one_tick(10, 4, 1.0)
    clean = elog.stream_log(10, 4, 0.1, T, ss, p, traj)
    iphi, ipose = 28 * 10 + 18 * 10 + 2, 28 * 10 + 4 * 10 + 5      # phi of stage 2; rotation-vector y of stage 5
    for arr, at, stage in (("traj", iphi, 2), ("traj", ipose, 5), ("ss", bstream.SS["PRREF"], 0), ("ss", bstream.SS["SECTOR"], None), ("p", 27, 0)):      # (p[27]: the measured rotation vector)
        a = dict(ss=ss.copy(), p=p.copy(), traj=traj.copy())
        a[arr][at] = np.nan
        row = elog.stream_log(10, 4, 0.1, T, a["ss"], a["p"], a["traj"])
        assert row[-4] == 10 and row[-3] == 0
        if stage is None:      # the window start is only used as a clamped table index
            continue
        assert not np.isfinite(row[stage * 88:(stage + 1) * 88]).all(), (arr, at)
    # an unusable n_valid word counts as "no plan"
    t2 = traj.copy(); t2[-4] = np.nan
    assert np.isnan(elog.stream_log(10, 4, 0.1, T, ss, p, t2)[:880]).all() and np.isfinite(clean[:880]).all()
