"""Batched receding-horizon streams: the whole tick of `BoundMPC.step()` on the device.

One stream = one trajectory (what one reference `BoundMPC` object is, BoundMPC.py:20-33 -- SURVEY.md 8b: "a
BoundMPC instance is stateful per trajectory").  The static part of a stream is its *path table* (the arrays
`ReferencePath.__init__` derives from the via points, ReferencePath.py:10-163), built here on the host once;
the dynamic part is the *stream state* (phi-state, rotation reference, window sector, error count, previous
solution).  Per tick the device runs  pack -> solve -> post  (csrc/bmpc_stream.inl + the solver kernel),
optionally as one captured hipGraph and optionally with the node's kinematic plant simulation, so a closed loop
needs no host round trip.  Re-planning (`BoundMPC.update`, BoundMPC.py:163-217): `StreamBatch.update` / `apply_update` write the
new path table and the state scalars update() sets, from then on the device takes the re-projection branch of step() (:335-369).
`StreamBatch.update_device` does the same on the device for the whole batch in one launch, from re-plan records (`replan_record`;
csrc/bmpc_stream_update.inl), without a synchronisation; `apply_update` is its specification.  The node's splice of the measured state into such a
record and disturbances of the plant are device code too (csrc/bmpc_stream_events.inl; mirrors `splice_record`, `disturb_robot`), on their own
launches (`update_device(splice=True)`, `disturb`) or as events behind the ticks of a rollout (`rollout(replan=, replan_tick=, disturb=)`).
The error bound itself -- how far the measured state of a tick is outside its tubes and joint limits, `tube_excess_of_state` on the host -- is
measured on the device as well (csrc/bmpc_stream_tube.inl): `StreamBatch.tube` behind a pack or a tick, `rollout(audit=, want_tube=)` inside a rollout.
"""
import ctypes

import numpy as np
from scipy.spatial.transform import Rotation as R

from . import _lib
from .solver import _give_start_rollout_back, _ptr, _stream_ptr, _take_start_rollout_off

# csrc/bmpc_stream.inl
PT = dict(P=0, IW=3, DPN=6, DR=9, RRV=12, PLO=15, PUP=17, RLO=19, RUP=21, BP1=23, BP2=26, BR1=29, BR2=32, CUM=35, EPMIN=36, ERMIN=37,
          EPMAX=38, ERMAX=39, S=40, LEN=48)
SS = dict(SECTOR=0, HASPREV=1, ERRCNT=2, PHI=3, DPHI=4, DDPHI=5, DDDPHI=6, PRREF=7, IWREF=10, PHIMAX=13, W=14, NENT=29, USINGPREV=30, VALID=31,
          PREV=32)
RB = dict(Q=0, DQ=7, DDQ=14, P=21, V=27, XPHID=33, JERK=36, LEN=43)


def ss_len(N):
    """[header 32 | previous solution 44 N | Cartesian pos, vel, acc, jerk of the previous plan 4 x 3 x N | updated flag | real-time continuation word |
    dphi_max | pad]"""
    return SS["PREV"] + 56 * N + 4


def ss_updated(N):
    return SS["PREV"] + 56 * N


def ss_dphimax(N):
    """dphi_max, the bound of the hard row dphi <= dphi_max: weights[4] of the CONSTRUCTOR (BoundMPC.py:77-79).  A re-plan replaces the weights and
    leaves this word, as the reference's update() does.  0 (a row not made by initial_state): stream_pack takes the current weights[4]."""
    return SS["PREV"] + 56 * N + 2


def path_table(rp, entries=None):
    """Flatten a host `ReferencePath` (boundmpc_amd.reference_path) into the device table [entries][48]."""
    M = len(rp.p)
    assert rp.phi_bias == 0
    n_rows = entries if entries is not None else M
    assert n_rows >= M
    T = np.zeros((n_rows, PT["LEN"]))
    at = lambda lst, j: lst[min(j, len(lst) - 1)]
    for j in range(M):
        e = T[j]
        e[0:3], e[3:6] = rp.p[j], at(rp.iw, j)
        dpj = at(rp.dp, j)
        e[6:9] = dpj / np.linalg.norm(dpj)
        e[9:12] = at(rp.dr, j)
        e[12:15] = R.from_matrix(at(rp.r, j)).as_rotvec()
        e[15:17], e[17:19] = at(rp.p_lower, j), at(rp.p_upper, j)
        e[19:21], e[21:23] = at(rp.r_lower, j), at(rp.r_upper, j)
        e[23:26], e[26:29], e[29:32], e[32:35] = at(rp.bp1, j), at(rp.bp2, j), at(rp.br1, j), at(rp.br2, j)
        e[35] = rp._cum[j]
        e[36], e[37], e[38], e[39], e[40] = at(rp.e_p_min, j), at(rp.e_r_min, j), at(rp.e_p_max, j), at(rp.e_r_max, j), at(rp.s, j)
    T[M:] = T[M - 1]
    return T, M


def initial_state(mpc, N):
    """Stream state of a freshly constructed host `BoundMPC` (before its first step)."""
    if getattr(mpc, "updated", False):
        raise ValueError("the host BoundMPC has been re-planned (update()): its warm start re-projects from Cartesian arrays the stream state does not "
                         "carry over; build the StreamBatch from a fresh object and call StreamBatch.update()")
    s = np.zeros(ss_len(N))
    s[SS["SECTOR"]] = mpc.ref_path.sector
    s[SS["PHI"]], s[SS["DPHI"]], s[SS["DDPHI"]], s[SS["DDDPHI"]] = mpc.phi_current[0], mpc.dphi_current[0], mpc.ddphi_current[0], mpc.dddphi_current[0]
    s[SS["PRREF"]:SS["PRREF"] + 3] = mpc.pr_ref
    s[SS["IWREF"]:SS["IWREF"] + 3] = mpc.iw_ref
    s[SS["PHIMAX"]] = mpc.phi_max[0]
    s[SS["W"]:SS["W"] + 15] = mpc.weights
    s[ss_dphimax(N)] = mpc.dphi_max[0]
    if mpc.prev_solution is not None:
        s[SS["HASPREV"]] = 1.0
        s[SS["PREV"]:SS["PREV"] + 44 * N] = np.asarray(mpc.prev_solution, dtype=float).ravel()
    s[SS["ERRCNT"]] = mpc.error_count
    return s


def apply_update(ss, N, S, pos_points, rot_points, pos_lim, rot_lim, bp1, br1, s, e_p_min, e_r_min, e_p_max, e_r_max, p, v, a, jerk, p0, weights,
                 entries=None):
    """Re-planning of one stream, the state part of BoundMPC.update() (BoundMPC.py:163-217) on the stream-state row `ss` (numpy,
    modified in place): new path table (returned, [entries][48]) and window start, path-parameter state projected onto the new first
    segment from the measured Cartesian state (p0, v, a, jerk), rotation reference, phi_max, weights, and the `updated` flag that
    switches the device's warm start to the re-projection branch of step() for good (the reference never clears it).  The previous
    solution, its Cartesian derivatives, dphi_max (ss_dphimax: the constructor's weights[4], NOT the new one) and the error count stay, as in the
    reference -- with one exception: a stream that had LOST its plan
    (error count >= N: the fused tick skips such a stream, status 3) is given a new attempt, its error count goes back to N - 1, so the tick after
    a re-planning solves it again on every launch shape (one more failure loses it again, a success resets the count as in BoundMPC.py:468)."""
    from .reference_path import ReferencePath
    from .bound_mpc import integrate_rotation_reference
    rp = ReferencePath(pos_points, rot_points, pos_lim, rot_lim, bp1, br1, s, e_p_min, e_r_min, e_p_max, e_r_max, S)
    if entries is not None and len(rp.p) > entries:
        raise ValueError(f"the new path has {len(rp.p)} table entries, the stream batch was built for {entries}: construct the StreamBatch "
                         "with the longest path it will ever follow")
    T, M = path_table(rp, entries)
    dp0 = rp.dp[0] / np.linalg.norm(rp.dp[0])
    phi = float((np.asarray(p0, dtype=float)[:3] - np.asarray(pos_points[0], dtype=float)) @ dp0)
    dpn = rp.dpd[:3, 0]
    ss[SS["SECTOR"]] = rp.sector
    ss[SS["PHI"]], ss[SS["DPHI"]], ss[SS["DDPHI"]], ss[SS["DDDPHI"]] = phi, float(v[:3] @ dpn), float(a[:3] @ dpn), float(jerk[:3] @ dpn)
    ss[SS["PRREF"]:SS["PRREF"] + 3] = integrate_rotation_reference(R.from_matrix(rot_points[0]).as_rotvec(), rp.dr[0], 0.0, phi)
    ss[SS["IWREF"]:SS["IWREF"] + 3] = rp.pd[3:, 0] + phi * rp.dpd[3:, 0]
    ss[SS["PHIMAX"]] = rp.phi_max - 0.0001
    ss[SS["W"]:SS["W"] + 15] = np.asarray(weights, dtype=float)
    ss[SS["NENT"]] = M
    ss[ss_updated(N)] = 1.0
    if ss[SS["ERRCNT"]] >= N:
        ss[SS["ERRCNT"]] = N - 1
    return T, M


# csrc/bmpc_stream_update.inl: the re-plan record [header 32 | n_max via entries of 32]
RP = dict(FLAG=0, N=1, NB=2, P0=3, V=6, A=9, JERK=12, W=15, HEAD=32)
RV = dict(P=0, R=3, PLO=12, PUP=14, RLO=16, RUP=18, BP1=20, BR1=23, S=26, EPMIN=27, ERMIN=28, EPMAX=29, ERMAX=30, LEN=32)


def replan_len(S, entries):
    """length of a re-plan record for a path table of `entries` rows: a path of n via points fills n + S - 1 of them"""
    return RP["HEAD"] + RV["LEN"] * (entries - S + 1)


def replan_record(S, entries, pos_points, rot_points, pos_lim, rot_lim, bp1, br1, s, e_p_min, e_r_min, e_p_max, e_r_max, p, v, a, jerk, p0, weights):
    """The re-plan record of one stream for bmpc_stream_update (StreamBatch.update_device): a numpy row [replan_len(S, entries)] with the flag
    raised.  Arguments as apply_update after (ss, N, S); rot_points are rotation matrices.  Limit and scalar lists shorter than the via-point list
    are extended by their last entry, as ReferencePath pads them; len(bp1) basis entries are computed on the device, the last one serves the rest.
    Contract of the frames: every table entry's error-plane basis must be orthonormal to its own segment -- (bp1, bp2) to the segment's direction,
    (br1, br2) to its rotation axis.  A basis entry that is replicated onto later segments (len(bp1) < n) is Gram-Schmidt'ed against ITS segment only:
    on a later segment with another direction the frame [br2, d, br1] is then not orthogonal, stream_pack reads its zyx angles through a normalised
    quaternion where the host mirror (scipy from_matrix) takes the nearest rotation, and v1..v3, ipar, io1, io2 of p differ between the two by
    O(1).  Give one basis vector per via point unless the segments behind the last one share its direction and axis.
    Raises the ValueError of apply_update when the path does not fit into `entries`."""
    n, nb = len(pos_points), len(bp1)
    if n + S - 1 > entries:
        raise ValueError(f"the new path has {n + S - 1} table entries, the stream batch was built for {entries}: construct the StreamBatch "
                         "with the longest path it will ever follow")
    if n < 2 or len(rot_points) != n or not 1 <= nb <= n or len(br1) != nb:
        raise ValueError(f"a path needs at least two via points, one rotation each and 1..n basis vectors (n = {n}, rotations {len(rot_points)}, "
                         f"bp1 {nb}, br1 {len(br1)})")
    rec = np.zeros(replan_len(S, entries))
    rec[RP["FLAG"]], rec[RP["N"]], rec[RP["NB"]] = 1.0, n, nb
    for key, val in (("P0", p0), ("V", v), ("A", a), ("JERK", jerk)):
        rec[RP[key]:RP[key] + 3] = np.asarray(val, dtype=float)[:3]
    rec[RP["W"]:RP["W"] + 15] = np.asarray(weights, dtype=float)
    via = rec[RP["HEAD"]:RP["HEAD"] + n * RV["LEN"]].reshape(n, RV["LEN"])
    at = lambda lst, j: lst[min(j, len(lst) - 1)]
    for j in range(n):
        e = via[j]
        e[RV["P"]:RV["P"] + 3] = pos_points[j]
        e[RV["R"]:RV["R"] + 9] = np.asarray(rot_points[j], dtype=float).reshape(9)
        e[RV["PLO"]:RV["PLO"] + 2], e[RV["PUP"]:RV["PUP"] + 2] = at(pos_lim[0], j), at(pos_lim[1], j)
        e[RV["RLO"]:RV["RLO"] + 2], e[RV["RUP"]:RV["RUP"] + 2] = at(rot_lim[0], j), at(rot_lim[1], j)
        if j < nb:
            e[RV["BP1"]:RV["BP1"] + 3], e[RV["BR1"]:RV["BR1"] + 3] = bp1[j], br1[j]
        e[RV["S"]], e[RV["EPMIN"]], e[RV["ERMIN"]], e[RV["EPMAX"]], e[RV["ERMAX"]] = at(s, j), at(e_p_min, j), at(e_r_min, j), at(e_p_max, j), at(e_r_max, j)
    return rec


def splice_record(rec, robot_row, dt, S, poor_bounds=False):
    """The device splice (csrc/bmpc_stream_events.inl stream_splice; bmpc_stream_update flags bit 1) as numpy over `RobotModel`: the words of a raised,
    valid re-plan record that the node takes from the plant (bound_mpc_node.py:121-137,158-162), from the robot record `robot_row` behind a post.
    Returns the spliced copy of `rec`: via[0].p = p_lie[:3] + 0.5 dt v[:3] (poor_bounds: the node's scenario 0, z lowered by 0.05 when v[2] < 0 and
    p_lie[1] * via[1].p[1] < 0), via[0].R = the matrix of the rotation vector p_lie[3:], header p0 = p_lie[:3], v = v[:3], a = J ddq + dJ dq,
    jerk = J u + 2 dJ ddq + ddJ dq (linear rows) -- the time derivative of a, where the node's j_cart (integrate_joint) takes ddJ at the state before
    the plant step and J ddq in the place of J u.  A record whose flag is 0 and an invalid record (bmpc_stream_update: info 1) come back unchanged."""
    from .robot_model import RobotModel
    rec, rb = np.array(rec, dtype=float), np.asarray(robot_row, dtype=float)
    n_max = (rec.shape[0] - RP["HEAD"]) // RV["LEN"]
    n, nb = rec[RP["N"]], rec[RP["NB"]]
    if rec[RP["FLAG"]] == 0.0 or not (2.0 <= n <= n_max) or not (1.0 <= nb <= int(n)):
        return rec
    model = RobotModel()
    q, dq, ddq, u = rb[RB["Q"]:RB["Q"] + 7], rb[RB["DQ"]:RB["DQ"] + 7], rb[RB["DDQ"]:RB["DDQ"] + 7], rb[RB["JERK"]:RB["JERK"] + 7]
    p_lie, v = rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6]
    _, J, dJ = model.forward_kinematics(q, dq)
    ddJ = model.ddjacobian_fk(q, dq, ddq)
    via = rec[RP["HEAD"]:].reshape(-1, RV["LEN"])
    lower = bool(poor_bounds) and v[2] < 0 and p_lie[1] * via[1, RV["P"] + 1] < 0
    via[0, RV["P"]:RV["P"] + 3] = p_lie[:3] + 0.5 * dt * v[:3]
    if lower:
        via[0, RV["P"] + 2] -= 0.05
    via[0, RV["R"]:RV["R"] + 9] = R.from_rotvec(p_lie[3:]).as_matrix().reshape(9)
    rec[RP["P0"]:RP["P0"] + 3], rec[RP["V"]:RP["V"] + 3] = p_lie[:3], v[:3]
    rec[RP["A"]:RP["A"] + 3] = (J @ ddq + dJ @ dq)[:3]
    rec[RP["JERK"]:RP["JERK"] + 3] = (J @ u + 2 * dJ @ ddq + ddJ @ dq)[:3]
    return rec


# csrc/bmpc_stream_events.inl: a disturbance row [delta q 7 | delta dq 7 | delta ddq 7]
DIST_LEN = 21


def disturb_robot(robot_row, d):
    """The device disturbance (stream_disturb; bmpc_stream_disturb) as numpy over `RobotModel`: d [DIST_LEN] added to q, dq, ddq of the robot record,
    p_lie and v recomputed from the disturbed joint state.  Non-finite entries count as 0, an all-zero row returns the record unchanged.  Returns a copy."""
    from .robot_model import RobotModel
    rb, d = np.array(robot_row, dtype=float), np.asarray(d, dtype=float)
    assert d.shape == (DIST_LEN,)
    d = np.where(np.isfinite(d), d, 0.0)
    if not d.any():
        return rb
    rb[RB["Q"]:RB["Q"] + 21] += d
    p, J, _ = RobotModel().forward_kinematics(rb[RB["Q"]:RB["Q"] + 7], rb[RB["DQ"]:RB["DQ"] + 7])
    rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = p, J @ rb[RB["DQ"]:RB["DQ"] + 7]
    return rb


def _poff(S):
    """Offsets of the parameter vector p (casadi_ocp_formulation.py:361-376; the same map as make_poff in csrc/bmpc_wave.inl)."""
    o, c = {}, 0
    for k, n in (("q0", 7), ("dq0", 7), ("ddq0", 7), ("phi0", 3), ("p0", 6), ("v0", 6), ("iwref0", 3), ("dtau", 3), ("ipar", 3 * S), ("io1", 3 * S), ("io2", 3 * S),
                 ("xphid", 3), ("jerk", 7), ("jerkphi", 1), ("sw", S + 1), ("jacr", 9), ("jacl", 9), ("pref", 6 * S), ("dpref", 6 * S), ("dpn", 3 * S),
                 ("bp1", 3 * S), ("bp2", 3 * S), ("br1", 3 * S), ("br2", 3 * S), ("a4", 9 * (S + 1)), ("a3", 9 * (S + 1)), ("a2", 9 * (S + 1)),
                 ("a1", 9 * (S + 1)), ("a0", 9 * (S + 1)), ("w", 15), ("phimax", 1), ("dphimax", 1), ("v1", 3 * S), ("v2", 3 * S), ("v3", 3 * S), ("qd", 7)):
        o[k] = c; c += n
    o["size"] = c
    return o


def tube_excess_of_state(p, S=4, rows=False):
    """BoundMPC's contract is the error bound: how far is the MEASURED state of a tick outside its tubes?  `p` [B][n_p] are the parameter vectors
    packed for a tick (device or host copies of what bmpc_stream_pack wrote): they hold the measured pose p0, the path parameter phi0 and the
    window of the path with its tube quartics, i.e. everything the five tube rows of casadi_ocp_formulation.py:316-349 need -- evaluated here at
    NODE 0, the state the plant is in (the NLP constrains nodes 1..N: node 0 is where the previous plans have taken the plant).  At node 0 the
    orientation-error components are the packed init_par / init_orth1 / init_orth2 of the current segment (compute_initial_rot_errors,
    util_functions.py:11-31: the exact zyx split of the measured orientation error), the position error is p0 - p_d(phi0).
    Returns (excess_pos [B][2], excess_rot [B][3]) in the LINEAR form |l_m| - |w_m| (metres, radians; <= 0: inside): position rows along bp1, bp2
    (rows 39, 40 of a stage), orientation rows tangential, br1, br2 (rows 38, 41, 42).  rows=True: (l [B][5], w [B][5]) in the row order 38..42
    instead (the reference's rows are l^2 - w^2)."""
    p = np.atleast_2d(np.asarray(p, dtype=float))
    o, B = _poff(S), len(p)
    want_rows, rows = rows, np.arange(B)
    sw = p[:, o["sw"]:o["sw"] + S + 1]
    phi = p[:, o["phi0"]]
    seg = np.full(B, S - 1)
    for i in range(S - 2, -1, -1):      # bound_mpc_functions.py:13-20
        seg = np.where(phi < sw[:, i + 1], i, seg)
    segb = np.minimum(seg, max(S - 2, 0))      # bp1 / bp2 never select the last window segment (:34-40)
    x = phi - sw[rows, seg]
    col = lambda key, n, sg: np.stack([p[rows, o[key] + c * S + sg] for c in range(n)], axis=1)      # [coord][seg] blocks
    b = np.zeros((B, 9))
    for ch in range(9):
        a4, a3, a2, a1, a0 = (p[rows, o[k] + ch * (S + 1) + seg] for k in ("a4", "a3", "a2", "a1", "a0"))
        b[:, ch] = (((a4 * x + a3) * x + a2) * x + a1) * x + a0
    pref, dpref = col("pref", 6, seg), col("dpref", 6, seg)
    e_p = p[:, o["p0"]:o["p0"] + 3] - (pref[:, :3] + dpref[:, :3] * x[:, None])
    bp = (col("bp1", 3, segb), col("bp2", 3, segb))
    l, w = np.zeros((B, 5)), np.zeros((B, 5))
    for m in range(2):
        off, hw = 0.5 * (b[:, m] + b[:, 2 + m]), 0.5 * (b[:, m] - b[:, 2 + m])
        l[:, 1 + m], w[:, 1 + m] = np.einsum("bi,bi->b", e_p, bp[m]) - off, hw
    dn, br1, br2 = col("dpn", 3, seg), col("br1", 3, seg), col("br2", 3, seg)
    ini = lambda key: np.stack([p[rows, o[key] + 3 * seg + c] for c in range(3)], axis=1)      # [seg][xyz] blocks
    ipar, io1, io2 = ini("ipar"), ini("io1"), ini("io2")
    l[:, 0], w[:, 0] = np.einsum("bi,bi->b", dn, ipar), b[:, 8]
    for m, (br, io) in enumerate(((br1, io1), (br2, io2))):
        off, hw = 0.5 * (b[:, 4 + m] + b[:, 6 + m]), 0.5 * (b[:, 4 + m] - b[:, 6 + m])
        l[:, 3 + m], w[:, 3 + m] = np.einsum("bi,bi->b", br, io) - off, hw
    if want_rows:
        return l, w
    ex = np.abs(l) - np.abs(w)
    return ex[:, 1:3], ex[:, [0, 3, 4]]


def robot_record(q, dq, ddq, p_lie, v, x_phi_d, jerk):
    return np.concatenate([q, dq, ddq, p_lie, v, x_phi_d, jerk]).astype(float)


def unpack_traj(t, N):
    """Trajectory record -> the reference's traj_data dict (BoundMPC.py:757-770) + flags."""
    t = np.asarray(t)
    n = int(t[-4])
    o, out = 0, {}
    for k in ("q", "dq", "ddq", "dddq"):
        out[k] = t[o:o + 7 * N].reshape(7, N)[:, :n]; o += 7 * N
    for k in ("p", "v", "a"):
        out[k] = t[o:o + 6 * N].reshape(6, N)[:, :n]; o += 6 * N
    for k in ("phi", "dphi", "ddphi", "dddphi"):
        out[k] = t[o:o + N][:n]; o += N
    return out, dict(n_valid=n, using_previous=bool(t[-3]), success=bool(t[-2]), g_viol=float(t[-1]))


# csrc/bmpc_stream_log.inl: the keys of the reference's ref_data / err_data (BoundMPC.py:614-752) with their widths, in row order
LOG_REF = (("p", 6), ("dp", 6), ("ddp", 6), ("dp_normed", 3), ("r_par_bound", 1), ("bound_lower", 4), ("bound_upper", 4), ("e_p_off", 2), ("e_r_off", 2),
           ("bp1", 3), ("bp2", 3), ("br1", 3), ("br2", 3), ("v1", 3), ("v2", 3), ("v3", 3))
LOG_ERR = tuple((k, 3) for k in ("e_p", "de_p", "e_p_par", "e_p_orth", "de_p_par", "de_p_orth", "e_r", "de_r", "e_r_par", "e_r_orth1", "e_r_orth2"))
LOG_STAGE = sum(w for _, w in LOG_REF + LOG_ERR)


def log_len(N):
    """[N][LOG_STAGE] | n_valid | error_count | 2 pad"""
    return N * LOG_STAGE + 4


ROLLOUT_ENTRIES = ("bmpc_stream_rollout", "bmpc_stream_rollout_events", "bmpc_stream_rollout_audit", "bmpc_stream_rollout_log", "bmpc_stream_rollout_legs",
                   "bmpc_stream_rollout_tuned", "bmpc_stream_rollout_plant")      # by entry number (csrc/bmpc_args.h bmpc_rollout_level)


def rollout_entry(replan=False, replan_tick=False, disturb=False, audit=False, want_tube=False, want_log=False, track=False, legs=False, tune=False, plant=False):
    """The C ABI entry StreamBatch.rollout calls, from which of its argument groups are present (booleans; a combination its argument checks pass).  The
    entry decides the kernel that runs: the highest feature present names it; without a queue, a table or a plant it is the lowest entry that has an
    argument for everything asked."""
    if plant:
        return ROLLOUT_ENTRIES[6]
    if tune:
        return ROLLOUT_ENTRIES[5]
    if legs:
        return ROLLOUT_ENTRIES[4]
    if not (replan or replan_tick or disturb or audit or want_tube or want_log or track):
        return ROLLOUT_ENTRIES[0]
    return ROLLOUT_ENTRIES[3 if want_log or track else 2 if audit or want_tube else 1]


def rollout_log_len(stages):
    """a log row of a rollout, cut to the first `stages` stages of the plan: [stages][LOG_STAGE] | n_valid | error_count | 2 pad"""
    return int(stages) * LOG_STAGE + 4


def unpack_log(row, N, stages=None):
    """Log row (bmpc_stream_log) -> (ref_data, err_data), the reference's logging dictionaries as the host mirror returns them: lists of flat
    arrays, one entry per stage of the plan (n_valid of them).  (None, None) for a stream without a plan (n_valid == 0).
    stages: the row is a rollout's (StreamBatch.rollout(want_log=True, log_stages=stages)["log_hist"][t, b]), cut to the first `stages` stages: the
    lists hold min(n_valid, stages) entries (n_valid is the whole plan's); (None, None) also for the NaN row of a tick the stream did not run."""
    row = np.asarray(row)
    K = N if stages is None else int(stages)
    assert 1 <= K <= N and row.shape == (K * LOG_STAGE + 4,)
    if stages is not None and np.isnan(row[-4]):
        return None, None
    n = min(int(row[-4]), K)
    if n == 0:
        return None, None
    body, o, out = row[:K * LOG_STAGE].reshape(K, LOG_STAGE)[:n], 0, ({}, {})
    for d, keys in zip(out, (LOG_REF, LOG_ERR)):
        for k, w in keys:
            d[k] = [body[i, o:o + w].copy() for i in range(n)]; o += w
    return out


# csrc/bmpc_stream_log.inl: the tracking record of a rollout with the log (BMPC_TRACK_* of include/boundmpc_hip.h)
TRACK = dict(SAMPLES=0, MAX_EP_ORTH=1, TICK_EP_ORTH=2, SUMSQ_EP_ORTH=3, MAX_EP_PAR=4, TICK_EP_PAR=5, SUMSQ_EP_PAR=6, MAX_ER=7, TICK_ER=8, SUMSQ_ER=9,
             REPLAYED=10, LEN=12)
_TRACK_FIGURES = (("EP_ORTH", "e_p_orth"), ("EP_PAR", "e_p_par"), ("ER", "e_r"))


def track_len():
    """[samples | max, tick, sum of squares of ||e_p_orth|| | of ||e_p_par|| | of ||e_r|| | replayed | pad]"""
    return TRACK["LEN"]


def unpack_track(row):
    """Tracking record of a rollout (StreamBatch.rollout(track=True)["track"][b], numpy) -> dict: samples, and per figure (e_p_orth, e_p_par in
    metres, e_r in radians) max_<figure> (NaN: a non-finite sample; -inf: no sample), tick_<figure> (the first tick of the maximum, None: none),
    sumsq_<figure> and the convenience rms_<figure> = sqrt(sumsq / samples) (NaN without a sample); replayed: samples that replayed the previous plan."""
    row = np.asarray(row)
    assert row.shape == (TRACK["LEN"],)
    n = int(row[TRACK["SAMPLES"]])
    out = dict(samples=n, replayed=int(row[TRACK["REPLAYED"]]))
    for K, k in _TRACK_FIGURES:
        t = row[TRACK["TICK_" + K]]
        out["max_" + k], out["tick_" + k], out["sumsq_" + k] = float(row[TRACK["MAX_" + K]]), None if t < 0 else int(t), float(row[TRACK["SUMSQ_" + K]])
        out["rms_" + k] = float(np.sqrt(row[TRACK["SUMSQ_" + K]] / n)) if n else float("nan")
    return out


def track_of_rows(log_hist, hist):
    """The numpy specification of the tracking record: log_hist [T][B][rollout_log_len(stages)] and hist [T][B][rollout_len()] of ONE rollout (its own
    rows) -> track [B][12].  A tick is a sample when its row has n_valid >= 1 (a NaN row -- a tick the stream did not run -- has none); the figures are
    the norms sqrt((x x + y y) + z z) of e_p_orth, e_p_par and e_r of STAGE 0: the largest with its first tick (a non-finite norm makes it NaN for
    good, its tick the first such), the squares summed in tick order; replayed counts the samples whose hist row says using_previous."""
    log_hist, hist = np.asarray(log_hist, dtype=np.float64), np.asarray(hist, dtype=np.float64)
    T, B = log_hist.shape[:2]
    assert hist.shape[:2] == (T, B) and hist.shape[2] == ROLL["LEN"] and (log_hist.shape[2] - 4) % LOG_STAGE == 0
    w0 = sum(w for _, w in LOG_REF)
    at = {"e_p_par": w0 + 6, "e_p_orth": w0 + 9, "e_r": w0 + 18}
    out = np.zeros((B, TRACK["LEN"]))
    for b in range(B):
        r = out[b]
        for K, _ in _TRACK_FIGURES:
            r[TRACK["MAX_" + K]], r[TRACK["TICK_" + K]] = -np.inf, -1.0
        for t in range(T):
            if not log_hist[t, b, -4] >= 1.0:
                continue
            r[TRACK["SAMPLES"]] += 1.0
            if hist[t, b, ROLL["USINGPREV"]] > 0.0:
                r[TRACK["REPLAYED"]] += 1.0
            for K, k in _TRACK_FIGURES:
                x, y, z = log_hist[t, b, at[k]:at[k] + 3]
                sq = (x * x + y * y) + z * z
                nrm, mx = np.sqrt(sq), r[TRACK["MAX_" + K]]
                if (not np.isnan(mx)) if not np.isfinite(nrm) else nrm > mx:
                    r[TRACK["MAX_" + K]], r[TRACK["TICK_" + K]] = (nrm if np.isfinite(nrm) else np.nan), float(t)
                r[TRACK["SUMSQ_" + K]] += sq
    return out


# csrc/bmpc_rollout_kernel.inl: the history row of one tick of one stream (BMPC_ROLL_* of include/boundmpc_hip.h)
ROLL = dict(ROBOT=0, PHI=43, ERRCNT=44, ITERS=45, STATUS=46, KKT=47, NVALID=48, USINGPREV=49, SUCCESS=50, GVIOL=51, LEN=52)
# a mission (bmpc_stream_rollout_legs, BMPC_LEG_* of include/boundmpc_hip.h): the bits of a record's trigger word leg_on, and of leg_why, the conditions
# that held when the record fired
LEG = dict(AT_GOAL=1, ON_LOST=2, WHY_GOAL=1, WHY_LOST=2, WHY_TICK=4)
# a sweep (bmpc_stream_rollout_tuned, BMPC_TUNE_* of include/boundmpc_hip.h): the slots of a stream's row of controller settings; NaN = the handle's value
TUNE = dict(MAX_ITER=0, TOL=1, MU_INIT=2, MU_WARM=3, MU_MIN_FAC=4, SLACK_PUSH=5, BOUND_MARGIN=6, HOLD=7, LVL_C=8, LVL_LO=9, LVL_HI=10, RT_TOL=11, RT_ROW_CAP=12,
            STALL_WINDOW=13, LEN=16)
TUNE_CROSS = 15      # the bit of tune_info for the one test across slots: the level rule as resolved


def tune_len():
    return TUNE["LEN"]


def tune_slot_ok(name, v):
    """The validity rule of one slot that is not NaN (csrc/bmpc_args.h bmpc_tune_slot_ok, restated): the test of bmpc_create or of the setter that
    guards the same value."""
    v = float(v)
    if not (-np.finfo(np.float64).max <= v <= np.finfo(np.float64).max):
        return False
    if name == "MAX_ITER":
        return 1.0 <= v <= 100000.0 and float(int(v)) == v
    if name in ("TOL", "MU_INIT", "MU_WARM", "MU_MIN_FAC", "SLACK_PUSH", "RT_TOL"):
        return v > 0.0
    if name == "BOUND_MARGIN":
        return 0.0 <= v <= 0.5
    if name == "HOLD":
        return v == 0.0 or v == 1.0
    if name in ("LVL_C", "LVL_LO", "LVL_HI", "RT_ROW_CAP"):
        return v >= 0.0
    if name == "STALL_WINDOW":
        return 0.0 <= v <= 2147483646.0 and float(int(v)) == v and not int(v) & 1
    raise KeyError(name)


def tune_check(row, defaults=None):
    """What the device answers for `row` [TUNE_LEN] in tune_info: the bit mask of its invalid slots, bit TUNE_CROSS where the level rule as resolved fails
    (LVL_HI > 0 needs 0 < LVL_LO <= LVL_HI).  defaults: the row NaN slots resolve to (BatchedOCPSolver.tune_defaults); None: the cross-slot test runs on
    the slots that are given, a NaN level counting as fine."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (TUNE["LEN"],)
    bad = 0
    for name, k in TUNE.items():
        if name != "LEN" and not np.isnan(row[k]) and not tune_slot_ok(name, row[k]):
            bad |= 1 << k
    lo, hi = (row[TUNE[n]] if not np.isnan(row[TUNE[n]]) else (defaults[TUNE[n]] if defaults is not None else np.nan) for n in ("LVL_LO", "LVL_HI"))
    if not np.isnan(lo) and not np.isnan(hi) and hi > 0.0 and not (lo > 0.0 and lo <= hi):      # (a level only the handle knows: the device decides)
        bad |= 1 << TUNE_CROSS
    return bad


def tune_table(B, fixed_barrier=None, level_c=0.02, **columns):
    """The table of a sweep, [B][TUNE_LEN] float64 for StreamBatch.rollout(tune=...): per slot name (any case: max_iter=, tol=, mu_init=, mu_warm=,
    mu_min_fac=, slack_push=, bound_margin=, hold=, lvl_c=, lvl_lo=, lvl_hi=, rt_tol=, rt_row_cap=, stall_window=) a scalar or a length-B array; NaN
    (a slot not named, or an entry of an array) keeps the handle's value for that stream.
    fixed_barrier: one setting for every stream, or a LIST of B settings (None: nothing for that stream), each of which expands exactly as BatchedOCPSolver(fixed_barrier=...) does -- None: nothing; "auto": the pair
    (0.01, 0.1); a pair (lo, hi): HOLD 1, the level rule (level_c, lo, hi), MU_INIT hi, MU_WARM lo, MU_MIN_FAC lo / tol; a float f: one fixed level,
    HOLD 0, no level rule, MU_INIT = MU_WARM = f, MU_MIN_FAC f / tol.  It needs the stream's `tol` column (the constructor's own tol), and the slots
    it sets must not be named as well.
    Raises ValueError on what the device would refuse (tune_check without defaults)."""
    B = int(B)
    T = np.full((B, TUNE["LEN"]), np.nan)
    for name, col in columns.items():
        k = TUNE.get(name.upper())
        if k is None or name.upper() == "LEN":
            raise ValueError(f"no slot {name!r}: {', '.join(n.lower() for n in TUNE if n != 'LEN')}")
        col = np.asarray(col, dtype=np.float64)
        if col.ndim and col.shape != (B,):
            raise ValueError(f"{name} must be a scalar or [{B}], got {list(col.shape)}")
        T[:, k] = col
    if fixed_barrier is not None:
        per = fixed_barrier if isinstance(fixed_barrier, list) else [fixed_barrier] * B
        if len(per) != B:
            raise ValueError(f"fixed_barrier must be one setting or a list of {B}")
        sets = ("HOLD", "LVL_C", "LVL_LO", "LVL_HI", "MU_INIT", "MU_WARM", "MU_MIN_FAC")
        for b, fb in enumerate(per):
            if fb is None:
                continue
            if any(not np.isnan(T[b, TUNE[n]]) for n in sets):
                raise ValueError("fixed_barrier sets hold, lvl_*, mu_init, mu_warm and mu_min_fac itself")
            if np.isnan(T[b, TUNE["TOL"]]):
                raise ValueError("fixed_barrier needs the tol column: the final level is tol * mu_min_fac")
            auto = isinstance(fb, (str, tuple, list))
            if isinstance(fb, str) and fb != "auto":
                raise ValueError(f"fixed_barrier {fb!r}: 'auto', a pair (lo, hi) or a float")
            lo, hi = (0.01, 0.1) if isinstance(fb, str) else ((float(fb[0]), float(fb[1])) if auto else (float(fb),) * 2)
            rule = (float(level_c), lo, hi) if auto else (0.0, 0.0, 0.0)
            T[b, [TUNE[n] for n in sets]] = [1.0 if auto else 0.0, *rule, hi, lo, lo / T[b, TUNE["TOL"]]]
    for b in range(B):
        bad = tune_check(T[b])
        if bad:
            names = [n.lower() for n, k in TUNE.items() if n != "LEN" and bad >> k & 1] + (["the level rule (lvl_hi > 0 needs 0 < lvl_lo <= lvl_hi)"] if bad >> TUNE_CROSS & 1 else [])
            raise ValueError(f"tune row {b}: invalid {', '.join(names)}")
    return T


def unpack_tune(row):
    """A row of a sweep's table (tune_table(...)[b], rollout()["tune_used"][b], BatchedOCPSolver.tune_defaults(); numpy) -> dict of its slots by lower-case
    name: max_iter, hold and stall_window as int, the rest float; None for a slot that holds NaN."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (TUNE["LEN"],)
    ints = ("MAX_ITER", "HOLD", "STALL_WINDOW")
    return {n.lower(): (None if np.isnan(row[k]) else (int(row[k]) if n in ints and np.isfinite(row[k]) else float(row[k]))) for n, k in TUNE.items() if n != "LEN"}


# a plant model (bmpc_stream_rollout_plant, bmpc_stream_plant; BMPC_PLANT_* of include/boundmpc_hip.h): the slots of a stream's row -- the drive between
# the first planned jerk of a tick and the plant; NaN = the identity value --, of its state and of its record
PLANT = dict(GAIN=0, BIAS=7, LAG=14, SAT=15, DELAY=16, LEN=20)
PLANT_STATE = dict(ACT=0, CMD=7, LEN=16)
PLANT_REC = dict(SAMPLES=0, N_SAT=1, MAX_DU=2, TICK_DU=3, JOINT_DU=4, SUMSQ_DU=5, LEN=8)
_PLANT_SLOTS = 17      # the slots that are looked at: GAIN[7], BIAS[7], LAG, SAT, DELAY


def plant_identity():
    """the row every NaN slot resolves to: the plant that IS the model (pad words 0)"""
    row = np.zeros(PLANT["LEN"])
    row[PLANT["GAIN"]:PLANT["GAIN"] + 7], row[PLANT["LAG"]], row[PLANT["SAT"]] = 1.0, 1.0, np.inf
    return row


def plant_check(row):
    """What the device answers for `row` [PLANT_LEN] in plant_info (csrc/bmpc_args.h bmpc_plant_check, restated): the bit mask of its invalid slots, bit k =
    slot k.  A NaN slot is the identity and valid; GAIN and BIAS must be finite, 0 < LAG <= 1, SAT > 0 (+inf allowed), DELAY 0 or 1; the pad words are
    never looked at."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (PLANT["LEN"],)
    bad = 0
    for k in range(_PLANT_SLOTS):
        v = float(row[k])
        if np.isnan(v):
            continue
        if k < PLANT["LAG"]:
            ok = np.isfinite(v)
        elif k == PLANT["LAG"]:
            ok = 0.0 < v <= 1.0
        elif k == PLANT["SAT"]:
            ok = v > 0.0
        else:
            ok = v == 0.0 or v == 1.0
        if not ok:
            bad |= 1 << k
    return bad


def plant_table(B, gain=None, bias=None, lag=None, sat=None, delay=None):
    """The table of plant models, [B][PLANT_LEN] float64 for StreamBatch.rollout(plant=...) and plant_step: gain and bias a scalar, [7] or [B][7], lag, sat
    and delay a scalar or [B]; NaN (an argument not given, or an entry of an array) is the identity -- gain 1, bias 0, lag 1 (none), sat +inf (none),
    delay 0.  Raises ValueError on what the device would refuse (plant_check)."""
    B = int(B)
    T = np.full((B, PLANT["LEN"]), np.nan)
    for name, col, at, w in (("gain", gain, PLANT["GAIN"], 7), ("bias", bias, PLANT["BIAS"], 7), ("lag", lag, PLANT["LAG"], 1), ("sat", sat, PLANT["SAT"], 1),
                             ("delay", delay, PLANT["DELAY"], 1)):
        if col is None:
            continue
        col = np.asarray(col, dtype=np.float64)
        ok = (col.ndim == 0 or col.shape in ((7,), (B, 7))) if w == 7 else (col.ndim == 0 or col.shape == (B,))
        if not ok:
            raise ValueError(f"{name} must be a scalar, " + (f"[7] or [{B}][7]" if w == 7 else f"or [{B}]") + f", got {list(col.shape)}")
        T[:, at:at + w] = col if w == 7 or col.ndim == 0 else col[:, None]
    for b in range(B):
        bad = plant_check(T[b])
        if bad:
            raise ValueError(f"plant row {b}: invalid slots {[k for k in range(_PLANT_SLOTS) if bad >> k & 1]}")
    return T


def plant_state_of(robot):
    """The plant state of streams whose drive has settled on the jerk of their robot records: robot [B][RB_LEN] (or one row) -> [B][PLANT_STATE_LEN] (or one
    row) with ACT = CMD = that jerk, pad words 0.  What plant_step and rollout(plant=) start from."""
    rb = np.asarray(robot, dtype=np.float64)
    st = np.zeros(rb.shape[:-1] + (PLANT_STATE["LEN"],))
    st[..., PLANT_STATE["ACT"]:PLANT_STATE["ACT"] + 7] = st[..., PLANT_STATE["CMD"]:PLANT_STATE["CMD"] + 7] = rb[..., RB["JERK"]:RB["JERK"] + 7]
    return st


def plant_robot(robot_row, plant_row, state_row, h):
    """The device plant step (stream_plant; bmpc_stream_plant) as numpy over `RobotModel`, the specification of one step: robot_row is the record behind a
    post that stepped the plant, c = its jerk the command.  Per joint c' = CMD if DELAY else c, CMD = c; a = GAIN c' + BIAS; f = a if LAG == 1 else
    ACT + LAG (a - ACT), ACT = f; u = clip(f, -SAT, SAT) (a NaN passes); D = u - c; q += h^3/24 D, dq += h^2/6 D, ddq += h/2 D, jerk = u.  Where any
    D != 0, p_lie and v are recomputed from the new joint state; where every D == 0 the record is returned unchanged.
    -> (robot row, state row, D [7], clipped: some joint was) -- copies."""
    from .robot_model import RobotModel
    rb, st = np.array(robot_row, dtype=float), np.array(state_row, dtype=float)
    w = np.asarray(plant_row, dtype=float)
    assert w.shape == (PLANT["LEN"],) and st.shape == (PLANT_STATE["LEN"],) and plant_check(w) == 0
    w = np.where(np.isnan(w), plant_identity(), w)
    c = rb[RB["JERK"]:RB["JERK"] + 7].copy()
    act, cmd = st[PLANT_STATE["ACT"]:PLANT_STATE["ACT"] + 7].copy(), st[PLANT_STATE["CMD"]:PLANT_STATE["CMD"] + 7].copy()
    a = w[PLANT["GAIN"]:PLANT["GAIN"] + 7] * (cmd if w[PLANT["DELAY"]] == 1.0 else c) + w[PLANT["BIAS"]:PLANT["BIAS"] + 7]
    lag, sat = w[PLANT["LAG"]], w[PLANT["SAT"]]
    f = a if lag == 1.0 else act + lag * (a - act)
    u = np.where(f > sat, sat, np.where(f < -sat, -sat, f))
    st[PLANT_STATE["ACT"]:PLANT_STATE["ACT"] + 7], st[PLANT_STATE["CMD"]:PLANT_STATE["CMD"] + 7] = f, c
    D = u - c
    if (D != 0.0).any():
        rb[RB["Q"]:RB["Q"] + 7] += h * h * h / 24 * D
        rb[RB["DQ"]:RB["DQ"] + 7] += h * h / 6 * D
        rb[RB["DDQ"]:RB["DDQ"] + 7] += h / 2 * D
        rb[RB["JERK"]:RB["JERK"] + 7] = u
        p, J, _ = RobotModel().forward_kinematics(rb[RB["Q"]:RB["Q"] + 7], rb[RB["DQ"]:RB["DQ"] + 7])
        rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = p, J @ rb[RB["DQ"]:RB["DQ"] + 7]
    return rb, st, D, bool(((f > sat) | (f < -sat)).any())


def unpack_plant_rec(row):
    """A plant record (rollout()["plant_rec"][b], numpy) -> dict: samples (the plant steps taken), n_sat (the ticks on which some joint clipped), max_du (the
    largest |u - c|; None without a sample), tick_du and joint_du (its first tick and joint; None likewise), sumsq_du, rms_du (over samples x 7)."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (PLANT_REC["LEN"],)
    n = int(row[PLANT_REC["SAMPLES"]])
    return dict(samples=n, n_sat=int(row[PLANT_REC["N_SAT"]]), max_du=float(row[PLANT_REC["MAX_DU"]]) if n else None,
                tick_du=int(row[PLANT_REC["TICK_DU"]]) if n else None, joint_du=int(row[PLANT_REC["JOINT_DU"]]) if n else None,
                sumsq_du=float(row[PLANT_REC["SUMSQ_DU"]]), rms_du=float(np.sqrt(row[PLANT_REC["SUMSQ_DU"]] / (7 * n))) if n else None)


# a sensor model (bmpc_stream_rollout_sensor, bmpc_stream_sense, bmpc_stream_unsense; BMPC_SENSOR_* of include/boundmpc_hip.h): the slots of a stream's row --
# the measurement between the plant and what pack, solve and post of a tick read; NaN = the identity value, 0 --, of its state and of its record
SENSOR = dict(BIAS=0, RES=7, NQ=8, NDQ=9, NDDQ=10, HOLD=11, LEN=16)
SENSOR_STATE = dict(HELD=0, HAS=21, SAME=22, TRUTH=24, LEN=64)
SENSOR_REC = dict(SAMPLES=0, MAX_DQ=1, TICK_DQ=2, JOINT_DQ=3, MAX_DP=4, TICK_DP=5, SUMSQ_DQ=6, LEN=8)
_SENSOR_SLOTS = 12      # the slots that are looked at: BIAS[7], RES, NQ, NDQ, NDDQ, HOLD
_TRUTH_HEAD = RB["XPHID"]      # the truth kept in the state: the words Q..V of the robot record, then JERK


def sensor_check(row):
    """What the device answers for `row` [SENSOR_LEN] in sensor_info (csrc/bmpc_args.h bmpc_sensor_check, restated): the bit mask of its invalid slots, bit k =
    slot k.  A NaN slot is the identity and valid; BIAS must be finite, RES, NQ, NDQ and NDDQ finite and >= 0, HOLD 0 or 1; the pad words are never looked
    at."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (SENSOR["LEN"],)
    bad = 0
    for k in range(_SENSOR_SLOTS):
        v = float(row[k])
        if np.isnan(v):
            continue
        if k < SENSOR["RES"]:
            ok = np.isfinite(v)
        elif k < SENSOR["HOLD"]:
            ok = np.isfinite(v) and v >= 0.0
        else:
            ok = v == 0.0 or v == 1.0
        if not ok:
            bad |= 1 << k
    return bad


def sensor_table(B, bias=None, res=None, nq=None, ndq=None, nddq=None, hold=None):
    """The table of sensor models, [B][SENSOR_LEN] float64 for StreamBatch.rollout(sensor=...), sense and unsense: bias a scalar, [7] or [B][7] (encoder
    offsets, rad), res (the quantisation step of the joint positions, rad), nq, ndq, nddq (the scales of the noise rows) and hold a scalar or [B]; NaN (an
    argument not given, or an entry of an array) is the identity, 0.  Raises ValueError on what the device would refuse (sensor_check)."""
    B = int(B)
    T = np.full((B, SENSOR["LEN"]), np.nan)
    for name, col, at, w in (("bias", bias, SENSOR["BIAS"], 7), ("res", res, SENSOR["RES"], 1), ("nq", nq, SENSOR["NQ"], 1), ("ndq", ndq, SENSOR["NDQ"], 1),
                             ("nddq", nddq, SENSOR["NDDQ"], 1), ("hold", hold, SENSOR["HOLD"], 1)):
        if col is None:
            continue
        col = np.asarray(col, dtype=np.float64)
        ok = (col.ndim == 0 or col.shape in ((7,), (B, 7))) if w == 7 else (col.ndim == 0 or col.shape == (B,))
        if not ok:
            raise ValueError(f"{name} must be a scalar, " + (f"[7] or [{B}][7]" if w == 7 else f"or [{B}]") + f", got {list(col.shape)}")
        T[:, at:at + w] = col if w == 7 or col.ndim == 0 else col[:, None]
    for b in range(B):
        bad = sensor_check(T[b])
        if bad:
            raise ValueError(f"sensor row {b}: invalid slots {[k for k in range(_SENSOR_SLOTS) if bad >> k & 1]}")
    return T


def sense_robot(robot_row, sensor_row, state_row, noise_row=None):
    """The device sample (stream_sense; bmpc_stream_sense) as numpy over `RobotModel`, the specification of one sample: robot_row is the TRUE record ahead of
    a pack, noise_row [21] the tick's unit draws (None: zeros; a non-finite word counts as 0).  The truth (Q..V, JERK) goes into the state; per joint
    m_q = (q + BIAS) + NQ n, with RES > 0 then RES rint(m_q / RES) (half to even), m_dq = dq + NDQ n, m_ddq = ddq + NDDQ n; out = HELD if HOLD and HAS else
    m; HELD = m, HAS = 1; SAME = every word of out equals the truth's.  Where SAME is 0 the record's q, dq, ddq become out and p_lie and v are recomputed
    from them; where it is 1 the record is returned unchanged.
    -> (robot row: what the pack reads, state row, out - truth [21], ||p_m - p|| in metres) -- copies."""
    from .robot_model import RobotModel
    rb, st = np.array(robot_row, dtype=float), np.array(state_row, dtype=float)
    w = np.asarray(sensor_row, dtype=float)
    assert w.shape == (SENSOR["LEN"],) and st.shape == (SENSOR_STATE["LEN"],) and sensor_check(w) == 0
    w = np.where(np.isnan(w), 0.0, w)
    n = np.zeros(DIST_LEN) if noise_row is None else np.asarray(noise_row, dtype=float)
    n = np.where(np.isfinite(n), n, 0.0)
    T = SENSOR_STATE["TRUTH"]
    st[T:T + _TRUTH_HEAD], st[T + _TRUTH_HEAD:T + _TRUTH_HEAD + 7] = rb[:_TRUTH_HEAD], rb[RB["JERK"]:RB["JERK"] + 7]
    truth = rb[:DIST_LEN].copy()
    m = truth.copy()
    m[:7] = (truth[:7] + w[SENSOR["BIAS"]:SENSOR["BIAS"] + 7]) + w[SENSOR["NQ"]] * n[:7]
    if w[SENSOR["RES"]] > 0.0:
        m[:7] = w[SENSOR["RES"]] * np.rint(m[:7] / w[SENSOR["RES"]])
    m[7:14] = truth[7:14] + w[SENSOR["NDQ"]] * n[7:14]
    m[14:] = truth[14:] + w[SENSOR["NDDQ"]] * n[14:]
    H = SENSOR_STATE["HELD"]
    out = st[H:H + DIST_LEN].copy() if w[SENSOR["HOLD"]] == 1.0 and st[SENSOR_STATE["HAS"]] == 1.0 else m.copy()
    st[H:H + DIST_LEN], st[SENSOR_STATE["HAS"]] = m, 1.0
    same = bool((out == truth).all())
    st[SENSOR_STATE["SAME"]] = 1.0 if same else 0.0
    dp = 0.0
    if not same:
        p, J, _ = RobotModel().forward_kinematics(out[:7], out[7:14])
        dp = float(np.linalg.norm(p[:3] - rb[RB["P"]:RB["P"] + 3]))
        rb[:DIST_LEN] = out
        rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = p, J @ out[7:14]
    return rb, st, out - truth, dp


def truth_robot(robot_row, state_row, h, stepped=True):
    """The way back to the true plant behind a post (stream_truth; bmpc_stream_unsense) as numpy over `RobotModel`: robot_row is the record behind the post,
    state_row what sense_robot left, stepped whether the post stepped the record (error count < N behind it).  SAME == 1: the record unchanged.  Else, where
    stepped: with c the record's jerk (the first planned jerk), the TRUE q, dq, ddq take the model's chain step from the true jerk to c --
    q += h dq + h^2/2 ddq + h^3/8 u_t + h^3/24 c, dq += h ddq + h^2/3 u_t + h^2/6 c, ddq += h/2 (u_t + c) --, p_lie and v are recomputed; else the words
    Q..V are the truth's again.  -> the robot row, a copy."""
    from .robot_model import RobotModel
    rb, st = np.array(robot_row, dtype=float), np.asarray(state_row, dtype=float)
    assert st.shape == (SENSOR_STATE["LEN"],)
    if st[SENSOR_STATE["SAME"]] == 1.0:
        return rb
    tr = st[SENSOR_STATE["TRUTH"]:SENSOR_STATE["TRUTH"] + _TRUTH_HEAD + 7]
    if not stepped:
        rb[:_TRUTH_HEAD] = tr[:_TRUTH_HEAD]
        return rb
    q, dq, ddq, ut, c = tr[:7], tr[7:14], tr[14:21], tr[_TRUTH_HEAD:], rb[RB["JERK"]:RB["JERK"] + 7].copy()
    qn = q + h * dq + h * h / 2 * ddq + h * h * h / 8 * ut + h * h * h / 24 * c
    dqn = dq + h * ddq + h * h / 3 * ut + h * h / 6 * c
    ddqn = ddq + h / 2 * (ut + c)
    p, J, _ = RobotModel().forward_kinematics(qn, dqn)
    rb[RB["Q"]:RB["Q"] + 7], rb[RB["DQ"]:RB["DQ"] + 7], rb[RB["DDQ"]:RB["DDQ"] + 7] = qn, dqn, ddqn
    rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = p, J @ dqn
    return rb


def unpack_sensor_rec(row):
    """A sensor record (rollout()["sensor_rec"][b], numpy) -> dict: samples, max_dq (the largest |q_m - q|; None without a sample), tick_dq and joint_dq (its
    first tick and joint), max_dp (the largest ||p_m - p||, metres: what the audit's position excess can miss) and tick_dp, sumsq_dq, rms_dq (over
    samples x 7)."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (SENSOR_REC["LEN"],)
    n = int(row[SENSOR_REC["SAMPLES"]])
    return dict(samples=n, max_dq=float(row[SENSOR_REC["MAX_DQ"]]) if n else None, tick_dq=int(row[SENSOR_REC["TICK_DQ"]]) if n else None,
                joint_dq=int(row[SENSOR_REC["JOINT_DQ"]]) if n else None, max_dp=float(row[SENSOR_REC["MAX_DP"]]) if n else None,
                tick_dp=int(row[SENSOR_REC["TICK_DP"]]) if n else None, sumsq_dq=float(row[SENSOR_REC["SUMSQ_DQ"]]),
                rms_dq=float(np.sqrt(row[SENSOR_REC["SUMSQ_DQ"]] / (7 * n))) if n else None)


# a state observer (bmpc_stream_rollout_observer, bmpc_stream_observe; BMPC_OBSERVER_* of include/boundmpc_hip.h): the slots of a stream's row -- the
# predictor-corrector between the sensor's sample and what pack, solve and post of a tick read; NaN = the identity value --, of its state and of its record
OBSERVER = dict(LQ=0, LDQ=1, LDDQ=2, LEAD=3, GATE=4, LEN=8)
OBSERVER_STATE = dict(POST=0, JP=21, JL=28, HAS=35, LAGS=36, LEN=40)
OBSERVER_REC = dict(SAMPLES=0, N_REJ=1, MAX_DQ=2, TICK_DQ=3, JOINT_DQ=4, MAX_DP=5, TICK_DP=6, SUMSQ_DQ=7, LEN=8)
_OBSERVER_SLOTS = 5      # the slots that are looked at: LQ, LDQ, LDDQ, LEAD, GATE
_OBSERVER_IDENTITY = (1.0, 1.0, 1.0, 0.0, np.inf)


def observer_check(row):
    """What the device answers for `row` [OBSERVER_LEN] in observer_info (csrc/bmpc_args.h bmpc_observer_check, restated): the bit mask of its invalid slots,
    bit k = slot k.  A NaN slot is the identity and valid; the gains LQ, LDQ, LDDQ must lie in (0, 1], LEAD be 0 or 1, GATE be > 0 (+inf: no gate); the pad
    words are never looked at."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (OBSERVER["LEN"],)
    bad = 0
    for k in range(_OBSERVER_SLOTS):
        v = float(row[k])
        if np.isnan(v):
            continue
        if k < OBSERVER["LEAD"]:
            ok = 0.0 < v <= 1.0
        elif k == OBSERVER["LEAD"]:
            ok = v == 0.0 or v == 1.0
        else:
            ok = v > 0.0
        if not ok:
            bad |= 1 << k
    return bad


def observer_table(B, lq=None, ldq=None, lddq=None, lead=None, gate=None):
    """The table of state observers, [B][OBSERVER_LEN] float64 for StreamBatch.rollout(observer=...) and observe: lq, ldq, lddq (the correction gains on q, dq
    and ddq, in (0, 1]; 1: the estimate is the sample), lead (1: the sample is one tick old, the sensor's HOLD, and the corrected estimate is advanced one
    chain step) and gate (the innovation gate on the joint positions, rad; +inf: none) a scalar or [B]; NaN (an argument not given, or an entry of an array)
    is the identity.  Raises ValueError on what the device would refuse (observer_check)."""
    B = int(B)
    T = np.full((B, OBSERVER["LEN"]), np.nan)
    for name, col, at in (("lq", lq, OBSERVER["LQ"]), ("ldq", ldq, OBSERVER["LDQ"]), ("lddq", lddq, OBSERVER["LDDQ"]), ("lead", lead, OBSERVER["LEAD"]), ("gate", gate, OBSERVER["GATE"])):
        if col is None:
            continue
        col = np.asarray(col, dtype=np.float64)
        if not (col.ndim == 0 or col.shape == (B,)):
            raise ValueError(f"{name} must be a scalar or [{B}], got {list(col.shape)}")
        T[:, at] = col
    for b in range(B):
        bad = observer_check(T[b])
        if bad:
            raise ValueError(f"observer row {b}: invalid slots {[k for k in range(_OBSERVER_SLOTS) if bad >> k & 1]}")
    return T


def _observer_step(x, up, u, h):
    """the model's chain step (csrc/bmpc_stream.inl chain_step) of the 21 words q | dq | ddq from the jerk `up` to the jerk `u`, in its order of operations"""
    q, dq, ddq = x[:7], x[7:14], x[14:21]
    return np.concatenate((q + h * dq + h * h / 2 * ddq + h * h * h / 8 * up + h * h * h / 24 * u, dq + h * ddq + h * h / 3 * up + h * h / 6 * u, ddq + h / 2 * (up + u)))


def observe_robot(robot_row, sensor_row, state_row, observer_row, ostate_row, h, noise_row=None):
    """The device sample and estimate (stream_observe; bmpc_stream_observe) as numpy over `sense_robot`, THE SPECIFICATION of one observer step: robot_row is the
    TRUE record ahead of a pack, sensor_row, state_row and noise_row the arguments of sense_robot, which makes the sample m (behind the sensor's HOLD);
    observer_row [OBSERVER_LEN] and ostate_row [OBSERVER_STATE_LEN] the stream's observer row and state, h the handle's step.  With J the record's jerk and
    step = the model's chain step per joint:
      fresh (HAS == 0)   post = out = m;  POST = m, JP = JL = J, HAS = 1, LAGS = 0; no gate
      LEAD == 0          prior = step(POST, JP, J);  post = prior + L (m - prior), the word m itself where L == 1; a sample with any |m_q - prior_q| not <= GATE
                         (a NaN among them) is rejected: post = prior;  out = post;  POST = post, JP = JL = J, LAGS = 0
      LEAD == 1          prior = step(POST, JP, JL) if LAGS else POST (the sample's own time);  post as above;  out = step(post, JL if LAGS else JP, J);
                         POST = post, where LAGS was 1 JP = the old JL, then JL = J, LAGS = 1
    SAME of the sensor state is decided on out against the truth over all 21 words; where it is 0 the record's q, dq, ddq become out and p_lie and v are
    recomputed from them, where it is 1 the record is returned unchanged.  The observer is not told of a disturbance, a spliced re-plan or a post that exhausted
    the plan: the innovation pulls it back, the state is never reset.
    -> (robot row: what the pack reads, sensor state row, observer state row, m [21], out - truth [21], ||p_est - p|| in metres, m - truth [21],
        ||p_m - p||, rejected) -- copies."""
    from .robot_model import RobotModel
    rb = np.array(robot_row, dtype=float)
    o, ost = np.asarray(observer_row, dtype=float), np.array(ostate_row, dtype=float)
    assert o.shape == (OBSERVER["LEN"],) and ost.shape == (OBSERVER_STATE["LEN"],) and observer_check(o) == 0
    o = np.where(np.isnan(o[:_OBSERVER_SLOTS]), _OBSERVER_IDENTITY, o[:_OBSERVER_SLOTS])
    rb_s, st, d_s, dp_s = sense_robot(robot_row, sensor_row, state_row, noise_row)
    truth, J = rb[:DIST_LEN].copy(), rb[RB["JERK"]:RB["JERK"] + 7].copy()
    m = rb_s[:DIST_LEN].copy()      # (where the sample equals the truth sense_robot returns the record unchanged: its words ARE the sample)
    P, JP, JL, HAS, LAGS = (OBSERVER_STATE[k] for k in ("POST", "JP", "JL", "HAS", "LAGS"))
    rejected = False
    if ost[HAS] != 1.0:
        post = out = m.copy()
        ost[JP:JP + 7], ost[JL:JL + 7], ost[HAS], ost[LAGS] = J, J, 1.0, 0.0
    else:
        lead, lags = o[OBSERVER["LEAD"]] == 1.0, ost[LAGS] == 1.0
        jp, jl = ost[JP:JP + 7].copy(), ost[JL:JL + 7].copy()
        prior = ost[P:P + DIST_LEN].copy() if lead and not lags else _observer_step(ost[P:P + DIST_LEN], jp, jl if lead else J, h)
        rejected = not bool((np.abs(m[:7] - prior[:7]) <= o[OBSERVER["GATE"]]).all())
        L = np.repeat(o[:3], 7)
        with np.errstate(invalid="ignore"):
            post = prior.copy() if rejected else np.where(L == 1.0, m, prior + L * (m - prior))
        if not lead:
            out = post.copy()
            ost[JP:JP + 7], ost[JL:JL + 7], ost[LAGS] = J, J, 0.0
        else:
            out = _observer_step(post, jl if lags else jp, J, h)
            if lags:
                ost[JP:JP + 7] = jl
            ost[JL:JL + 7], ost[LAGS] = J, 1.0
    ost[P:P + DIST_LEN] = post
    same = bool((out == truth).all())
    st[SENSOR_STATE["SAME"]] = 1.0 if same else 0.0
    dp = 0.0
    if not same:
        p, Jac, _ = RobotModel().forward_kinematics(out[:7], out[7:14])
        dp = float(np.linalg.norm(p[:3] - rb[RB["P"]:RB["P"] + 3]))
        rb[:DIST_LEN] = out
        rb[RB["P"]:RB["P"] + 6], rb[RB["V"]:RB["V"] + 6] = p, Jac @ out[7:14]
    return rb, st, ost, m, out - truth, dp, d_s, dp_s, rejected


def unpack_observer_rec(row):
    """An observer record (rollout()["observer_rec"][b], numpy) -> dict: samples (the estimates made), n_rej (the samples the gate rejected), max_dq (the largest
    |q_est - q|; None without an estimate), tick_dq and joint_dq (its first tick and joint), max_dp (the largest ||p_est - p||, metres) and tick_dp, sumsq_dq,
    rms_dq (over samples x 7)."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (OBSERVER_REC["LEN"],)
    n = int(row[OBSERVER_REC["SAMPLES"]])
    return dict(samples=n, n_rej=int(row[OBSERVER_REC["N_REJ"]]), max_dq=float(row[OBSERVER_REC["MAX_DQ"]]) if n else None, tick_dq=int(row[OBSERVER_REC["TICK_DQ"]]) if n else None,
                joint_dq=int(row[OBSERVER_REC["JOINT_DQ"]]) if n else None, max_dp=float(row[OBSERVER_REC["MAX_DP"]]) if n else None,
                tick_dp=int(row[OBSERVER_REC["TICK_DP"]]) if n else None, sumsq_dq=float(row[OBSERVER_REC["SUMSQ_DQ"]]),
                rms_dq=float(np.sqrt(row[OBSERVER_REC["SUMSQ_DQ"]] / (7 * n))) if n else None)


def rollout_len():
    """[robot record 43 | phi | error count | iters | status | kkt | n_valid | using_previous | success | g_viol]"""
    return ROLL["LEN"]


def unpack_rollout(row):
    """History row of a rollout (StreamBatch.rollout()["hist"][t, b], numpy) -> dict: the fields of the robot record behind the tick's post
    (q, dq, ddq, p, v, x_phi_d, jerk) and the named scalars.  None for a tick the stream did not run (a NaN row)."""
    row = np.asarray(row)
    assert row.shape == (ROLL["LEN"],)
    if np.isnan(row[ROLL["STATUS"]]):
        return None
    names = [k for k in sorted(RB, key=RB.get) if k != "LEN"]
    out = {k.lower(): row[RB[k]:RB[names[i + 1]] if i + 1 < len(names) else RB["LEN"]].copy() for i, k in enumerate(names)}
    out["x_phi_d"] = out.pop("xphid")
    out.update(phi=float(row[ROLL["PHI"]]), error_count=int(row[ROLL["ERRCNT"]]), status=int(row[ROLL["STATUS"]]), kkt=float(row[ROLL["KKT"]]),
               iters=None if np.isnan(row[ROLL["ITERS"]]) else int(row[ROLL["ITERS"]]), n_valid=int(row[ROLL["NVALID"]]),
               using_previous=bool(row[ROLL["USINGPREV"]]), success=bool(row[ROLL["SUCCESS"]]), g_viol=float(row[ROLL["GVIOL"]]))
    return out


# csrc/bmpc_stream_tube.inl: the tube row of one stream (BMPC_TUBE_* of include/boundmpc_hip.h) and the audit record of a rollout (BMPC_AUDIT_*)
TUBE = dict(L=0, W=5, EX_POS=10, EX_ROT=11, EX_Q=12, EX_DQ=13, SEG=14, PHI=15, LEN=16)
AUDIT = dict(SAMPLES=0, MAX_POS=1, TICK_POS=2, MAX_ROT=3, TICK_ROT=4, MAX_Q=5, MAX_DQ=6, N_POS=7, N_ROT=8, N_JOINT=9, FIRST_OUT=10, LEN=12)


def tube_len():
    """[l 5 | w 5 | ex_pos | ex_rot | ex_q | ex_dq | segment | phi0]: `tube_excess_of_state` of one stream in both of its forms (rows 38..42:
    orientation tangential, position bp1, bp2, orientation br1, br2) and the joint figures max_j |q0_j| - qlim_j, max_j |dq0_j| - dqlim_j"""
    return TUBE["LEN"]


def unpack_audit(row):
    """Audit record of a rollout (StreamBatch.rollout(audit=True)["audit"][b], numpy) -> dict: samples, the largest position / orientation excess
    (metres, radians; <= 0: inside; NaN: a non-finite sample) with the tick each was measured AHEAD of (row t of tube_hist is the state tick t
    starts from), the largest joint figures, the counts of samples outside and first_out (None: never outside a tube).  A stream lost on entry
    has samples 0 and maxima -inf."""
    row = np.asarray(row)
    assert row.shape == (AUDIT["LEN"],)
    tick = lambda k: None if row[AUDIT[k]] < 0 else int(row[AUDIT[k]])
    return dict(samples=int(row[AUDIT["SAMPLES"]]), max_pos=float(row[AUDIT["MAX_POS"]]), tick_pos=tick("TICK_POS"), max_rot=float(row[AUDIT["MAX_ROT"]]),
                tick_rot=tick("TICK_ROT"), max_q=float(row[AUDIT["MAX_Q"]]), max_dq=float(row[AUDIT["MAX_DQ"]]), n_pos=int(row[AUDIT["N_POS"]]),
                n_rot=int(row[AUDIT["N_ROT"]]), n_joint=int(row[AUDIT["N_JOINT"]]), first_out=tick("FIRST_OUT"))


# Named reads of the stream records: pure indexing of the last axis, on numpy arrays and torch tensors alike (one row or a batch; no copy, no sync).
def applied(traj):
    """the success flag of a trajectory record (unpack_traj's `success`): the tick's plan was applied"""
    return traj[..., -2] > 0.5


def g_viol(traj):
    """the summed violation the acceptance rule judged (unpack_traj's `g_viol`)"""
    return traj[..., -1]


def has_plan(state, N):
    """error count < N: the stream still holds a plan (from N on the reference's step() returns None, BoundMPC.py:498-506, and the fused tick skips it)"""
    return state[..., SS["ERRCNT"]] < N


def valid(state):
    """the VALID word stream_post wrote: has_plan as of the last post"""
    return state[..., SS["VALID"]] > 0.5


def phi(state):
    return state[..., SS["PHI"]]


def level(dual, N):
    """the barrier level in the dual state [57 N multipliers | mu | ...]"""
    return dual[..., 57 * N]


def first_stage_tube_rows(g, N):
    """rows 38..42 of stage 0 of g [..][43 N]: the tube rows (l^2 - w^2; orientation tangential, position bp1, bp2, orientation br1, br2) of the state the plant reaches next"""
    assert g.shape[-1] == 43 * N
    return g[..., 38:43]


def set_continue_rejected(state, N, on=True):
    """the word behind the `updated` flag: "the last iterate was rejected: the next pack continues from xlast" (bmpc_stream_pack_rt)"""
    state[..., ss_updated(N) + 1] = 1.0 if on else 0.0


def tick_tube_figures(p, state, g, traj, N, S=4):
    """What a closed loop records per tick about the tubes, each [B], numpy: the largest position / orientation excess of the MEASURED state
    (tube_excess_of_state of the packed `p`; -inf where the stream has no plan: the fused tick skips it, its p is stale) and the largest
    position / orientation row of the plan's first stage (first_stage_tube_rows; -inf where the plan was not applied)."""
    cpu = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    ex_p, ex_r = tube_excess_of_state(cpu(p), S)
    plan, app, g0 = cpu(has_plan(state, N)), cpu(applied(traj)), cpu(first_stage_tube_rows(g, N))
    return (np.where(plan, ex_p.max(axis=1), -np.inf), np.where(plan, ex_r.max(axis=1), -np.inf),
            np.where(app, g0[:, 1:3].max(axis=1), -np.inf), np.where(app, g0[:, [0, 3, 4]].max(axis=1), -np.inf))


def tube_summary(tube_p, tube_r, row_p, row_r, tol=1e-6):
    """Summary of tick_tube_figures stacked over the ticks [ticks][B]: fractions of the plant samples outside, largest excess, streams ever outside,
    and the first-stage rows of the applied plans."""
    tube_p, tube_r, row_p, row_r = (np.asarray(a) for a in (tube_p, tube_r, row_p, row_r))
    n, n_app = int(np.isfinite(tube_p).sum()), int(np.isfinite(row_p).sum())
    return {"plant_samples": n, "tolerance": tol,
            "fraction_outside_the_position_tube": float((tube_p > tol).sum() / max(n, 1)), "largest_position_excess_m": float(max(tube_p.max(), 0.0)),
            "fraction_outside_the_orientation_tube": float((tube_r > tol).sum() / max(n, 1)), "largest_orientation_excess_rad": float(max(tube_r.max(), 0.0)),
            "streams_ever_outside_a_tube": int(((tube_p > tol) | (tube_r > tol)).any(axis=0).sum()),
            "applied_plans_first_stage_rows_reference_form": {
                "applied_plans": n_app, "fraction_with_a_position_row_above_1e-6": float((row_p > tol).sum() / max(n_app, 1)),
                "largest_position_row_m2": float(max(row_p.max(), 0.0)),
                "fraction_with_an_orientation_row_above_1e-6": float((row_r > tol).sum() / max(n_app, 1)),
                "largest_orientation_row_rad2": float(max(row_r.max(), 0.0))}}


class StreamBatch:
    """B streams on the GPU.  `mpcs`: list of freshly constructed host `boundmpc_amd.bound_mpc.BoundMPC` objects (used only to
    read their path and initial state; they are not advanced)."""

    def __init__(self, solver, mpcs, device="cuda"):
        import torch
        self.solver, self.B, self.N, self.S = solver, len(mpcs), solver.N, solver.S
        # the warm starts of a stream are the reference's own (stream_pack: its cold start or the shifted plan, BoundMPC.py:316-375): taken as given, also
        # by the stateless ticks (cold duals); on closed loops the rollout of a start that is off its dynamics costs plans (oracle/bmpc_oracle.c solve_one)
        # (a setting of the caller's handle: the previous value comes back in close(); an A/B library from before the option has no such entry point)
        self._rollout_was = _take_start_rollout_off(solver)
        lens = [ctypes.c_int() for _ in range(4)]
        _lib.check(solver._lib.bmpc_stream_lengths(solver._h, *[ctypes.byref(v) for v in lens]), "bmpc_stream_lengths")
        self.pt_len, self.ss_len, self.rb_len, self.tr_len = (v.value for v in lens)
        assert self.pt_len == PT["LEN"] and self.rb_len == RB["LEN"] and self.ss_len == ss_len(self.N)
        self.entries = max(len(m.ref_path.p) for m in mpcs)
        tabs, states = [], []
        for m in mpcs:
            assert m.N == self.N and m.nr_segs == self.S and abs(m.dt - solver.dt) < 1e-15
            T, M = path_table(m.ref_path, self.entries)
            s = initial_state(m, self.N); s[SS["NENT"]] = M
            tabs.append(T); states.append(s)
        t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
        self.path, self.state = t64(np.stack(tabs)), t64(np.stack(states))
        self.robot = torch.zeros((self.B, self.rb_len), dtype=torch.float64, device=device)
        self.p = torch.empty((self.B, solver.n_p), dtype=torch.float64, device=device)
        self.x0 = torch.empty((self.B, solver.n_w), dtype=torch.float64, device=device)
        self.dual = solver.new_state(self.B, device)
        self.x = torch.empty((self.B, solver.n_w), dtype=torch.float64, device=device)
        self.g = torch.empty((self.B, solver.n_g), dtype=torch.float64, device=device)
        self.iters = torch.zeros((self.B,), dtype=torch.int32, device=device)
        self.status = torch.zeros((self.B,), dtype=torch.int32, device=device)
        self.kkt = torch.zeros((self.B,), dtype=torch.float64, device=device)
        self.traj = torch.zeros((self.B, self.tr_len), dtype=torch.float64, device=device)
        self._graphs = {}
        self._log = None         # log(): allocated on first use
        self._tube = None        # tube(): allocated on first use
        self.replan = self.replan_info = None      # update_device(): record buffer [B][replan_len] and info [B], allocated on first use
        self.legs = None         # rollout(legs=...): queue buffer [B][K][replan_len], allocated on first use
        self.tick_ms = None      # closed_loop(timed=True): HIP-event time of the tick just run
        self.plant_state = None  # plant_step(), rollout(plant=...): the drives' state [B][PLANT_STATE_LEN], created from the robot records on first use
        self.plant_info = self.plant_rec = None      # plant_step(): masks [B] and accumulated records [B][PLANT_REC_LEN], allocated on first use
        self.sensor_state_ = None      # sense(), rollout(sensor=...): the sensors' state [B][SENSOR_STATE_LEN], zeros (fresh) on first use; read it with sensor_state()
        self.sensor_info = self.sensor_rec = self.meas = None      # sense(): masks [B], accumulated records [B][SENSOR_REC_LEN] and the record the pack reads, allocated on first use
        self.observer_state_ = None      # observe(), rollout(observer=...): the observers' state [B][OBSERVER_STATE_LEN], zeros (fresh) on first use; read it with observer_state()
        self.observer_info = self.observer_rec = self.sample = None      # observe(): masks [B], accumulated records [B][OBSERVER_REC_LEN] and the raw samples, allocated on first use
        solver._children.add(self)

    def update(self, b, *args, **kw):
        """Re-plan stream b: `apply_update` on a host copy of its state row, then the new table and state go back to the device
        (a rare event; the per-tick work stays on the device).  Arguments as apply_update after (ss, N, S)."""
        import torch
        torch.cuda.synchronize(self.state.device)
        row = self.state[b].cpu().numpy().copy()
        T, M = apply_update(row, self.N, self.S, *args, entries=self.entries, **kw)
        self.path[b].copy_(torch.as_tensor(T, dtype=torch.float64))
        self.state[b].copy_(torch.as_tensor(row, dtype=torch.float64))
        return float(row[SS["PHIMAX"]])

    def _replan_buffer(self, records, stream):
        """the device record buffer (allocated on first use) holding `records`; `self.replan` itself is taken as it is"""
        import torch
        if self.replan is None:
            n = self.solver._lib.bmpc_stream_replan_len(self.solver._h, self.entries)
            assert n == replan_len(self.S, self.entries)
            self.replan = torch.zeros((self.B, n), dtype=torch.float64, device=self.path.device)
            self.replan_info = torch.zeros((self.B,), dtype=torch.int32, device=self.path.device)
        if records is not self.replan:
            if not torch.is_tensor(records):
                records = torch.as_tensor(np.ascontiguousarray(records, dtype=np.float64))
            if tuple(records.shape) != tuple(self.replan.shape):
                raise ValueError(f"records must be [{self.B}][{self.replan.shape[1]}] (replan_len(S, entries)), got {tuple(records.shape)}")
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):      # the copy ahead of the launch, same stream
                self.replan.copy_(records)
        return self.replan

    def _legs_buffer(self, records, stream):
        """the device queue buffer `self.legs` [B][K][replan_len] (allocated on first use and whenever K changes) holding `records`: a tensor or an array
        of that shape, or B lists of K `replan_record` rows; `self.legs` itself is taken as it is.  -> K"""
        import torch
        if records is self.legs and records is not None:
            return int(self.legs.shape[1])
        if not torch.is_tensor(records):
            records = torch.as_tensor(np.ascontiguousarray(records, dtype=np.float64))
        n = self.solver._lib.bmpc_stream_replan_len(self.solver._h, self.entries)
        assert n == replan_len(self.S, self.entries)
        if records.ndim != 3 or records.shape[0] != self.B or records.shape[1] < 1 or records.shape[2] != n:
            raise ValueError(f"legs must be [{self.B}][K >= 1][{n}] (replan_len(S, entries)), got {list(records.shape)}")
        if self.legs is None or tuple(self.legs.shape) != tuple(records.shape):
            self.legs = torch.zeros(tuple(records.shape), dtype=torch.float64, device=self.path.device)
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):      # the copy ahead of the launch, same stream
            self.legs.copy_(records)
        return int(self.legs.shape[1])

    @staticmethod
    def _update_flags(set_goal, splice, poor_bounds):
        if poor_bounds and not splice:
            raise ValueError("poor_bounds is a rule of the splice (splice=True)")
        return int(bool(set_goal)) | (2 if splice else 0) | (4 if poor_bounds else 0)

    def update_device(self, records, set_goal=True, stream=None, splice=False, poor_bounds=False):
        """Re-plan on the device (bmpc_stream_update): `records` [B][replan_len(S, entries)], a tensor or an array of `replan_record` rows; a
        row whose flag is 0 leaves its stream alone.  One launch over the batch, asynchronous on `stream`, no synchronisation and no host copy of
        the state: call it after post(), tick(), tick_graph() or log() and before the next pack.  The records are copied into a device buffer
        allocated on first use (`self.replan`; a caller that captures the launch raises flags in that buffer, the launch clears them) -- passing
        `self.replan` itself copies nothing.  set_goal: also robot[x_phi_d] = (phi_max, 0, 0), as the node does right after update().
        splice: the device first writes what the node takes from the plant into every raised record, from the stream's robot record (the first via
        point, p0, v, a, jerk: `splice_record` is the mirror; poor_bounds: the node's scenario-0 rule with it); the spliced words stay in `self.replan`.
        Returns the `info` tensor [B] (int32; 1: invalid record, stream untouched), valid once `stream` has run the launch."""
        flags = self._update_flags(set_goal, splice, poor_bounds)
        self._replan_buffer(records, stream)
        _lib.check(self.solver._lib.bmpc_stream_update(self.solver._h, self.B, _ptr(self.replan), _ptr(self.path), self.entries, _ptr(self.state), _ptr(self.robot),
                                                       _ptr(self.replan_info), flags, self._stream(stream)), "bmpc_stream_update")
        return self.replan_info

    def disturb(self, d, stream=None):
        """Disturb the plants (bmpc_stream_disturb): d [B][DIST_LEN] (tensor or array) = delta q | delta dq | delta ddq, added to the robot records;
        pose and Cartesian velocity follow (`disturb_robot` is the mirror).  Between a tick's post (or log, or update) and the next pack; one launch,
        asynchronous on `stream`."""
        assert self.solver._lib.bmpc_stream_disturb_len() == DIST_LEN
        d = self._dev64(d, (self.B, DIST_LEN), "d", stream)
        _lib.check(self.solver._lib.bmpc_stream_disturb(self.solver._h, self.B, _ptr(self.robot), _ptr(d), self._stream(stream)), "bmpc_stream_disturb")

    def _plant_state(self, stream):
        """the drives' state on the device; on first use ACT = CMD = the jerk of the robot records as they are now (plant_state_of, on `stream`)"""
        import torch
        if self.plant_state is None:
            lib = self.solver._lib
            assert (lib.bmpc_stream_plant_len(), lib.bmpc_stream_plant_state_len(), lib.bmpc_stream_plant_rec_len()) == (PLANT["LEN"], PLANT_STATE["LEN"], PLANT_REC["LEN"])
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
                self.plant_state = torch.zeros((self.B, PLANT_STATE["LEN"]), dtype=torch.float64, device=self.path.device)
                for at in (PLANT_STATE["ACT"], PLANT_STATE["CMD"]):
                    self.plant_state[:, at:at + 7] = self.robot[:, RB["JERK"]:RB["JERK"] + 7]
        return self.plant_state

    def plant_reset(self, stream=None):
        """Start the drives afresh: `self.plant_state` from the robot records as they are NOW (ACT = CMD = their jerk, plant_state_of) and an empty
        `self.plant_rec`.  A per-tick loop that is to leave what rollout(plant=) leaves calls it where that launch would start: ahead of the first tick."""
        self.plant_state = self.plant_rec = self.plant_info = None
        return self._plant_state(stream)

    def plant_step(self, plant, tick=0, stream=None):
        """The drives between the commands and the plants, one step (bmpc_stream_plant): plant [B][PLANT_LEN] (`plant_table(B, ...)`, an array or a device
        tensor, taken as it is), row b the actuator model of stream b.  Call it behind tick() (or post()) and AHEAD of log(), tube of the next tick, disturb()
        and update_device(): it corrects the robot records from the plant the post stepped with the planned jerk to the plant under the jerk the drive
        delivers (`plant_robot` is the mirror).  A stream without a plan is skipped; a stream with an invalid row is left alone, its mask in the result.
        Keeps `self.plant_state` (created from the robot records as they are on first use -- behind the first tick of a loop, unless plant_reset() was called
        ahead of it, which is where rollout(plant=) creates it) and accumulates `self.plant_rec`
        [B][PLANT_REC_LEN] (slots PLANT_REC; `tick` is what its TICK_DU names), initialised on first use.  One launch, asynchronous on `stream`, capturable.
        Returns the `plant_info` tensor [B] (int32), valid once `stream` has run the launch."""
        import torch
        plant = self._dev64(plant, (self.B, PLANT["LEN"]), "plant", stream)
        state = self._plant_state(stream)
        if self.plant_rec is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
                self.plant_info = torch.zeros((self.B,), dtype=torch.int32, device=self.path.device)
                rec0 = np.zeros(PLANT_REC["LEN"]); rec0[PLANT_REC["MAX_DU"]], rec0[PLANT_REC["TICK_DU"]], rec0[PLANT_REC["JOINT_DU"]] = -np.inf, -1.0, -1.0
                self.plant_rec = torch.as_tensor(rec0).to(self.path.device).repeat(self.B, 1).contiguous()
        _lib.check(self.solver._lib.bmpc_stream_plant(self.solver._h, self.B, _ptr(self.robot), _ptr(self.state), _ptr(plant), _ptr(state), _ptr(self.plant_info),
                                                      _ptr(self.plant_rec), int(tick), self._stream(stream)), "bmpc_stream_plant")
        self._plant_input = plant      # the launch is asynchronous: its input lives until the next one replaces it
        return self.plant_info

    def sensor_state(self, stream=None):
        """the sensors' state on the device, [B][SENSOR_STATE_LEN] (slots SENSOR_STATE): the held sample, and the truth while a tick is in flight; zeros
        (fresh: no sample held) on first use, then carried from launch to launch, so rollouts chain"""
        import torch
        if self.sensor_state_ is None:
            lib = self.solver._lib
            assert (lib.bmpc_stream_sensor_len(), lib.bmpc_stream_sensor_state_len(), lib.bmpc_stream_sensor_rec_len()) == (SENSOR["LEN"], SENSOR_STATE["LEN"], SENSOR_REC["LEN"])
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
                self.sensor_state_ = torch.zeros((self.B, SENSOR_STATE["LEN"]), dtype=torch.float64, device=self.path.device)
        return self.sensor_state_

    def sensor_reset(self, stream=None):
        """Start the sensors afresh: a state of zeros (no sample held) and an empty `self.sensor_rec`.  A per-tick loop that is to leave what
        rollout(sensor=) leaves calls it where that launch would start."""
        self.sensor_state_ = self.sensor_rec = self.sensor_info = self.meas = None
        return self.sensor_state(stream)

    def sense(self, sensor, noise=None, tick=0, stream=None):
        """The sensors between the plants and the controller, the sample of one tick (bmpc_stream_sense): sensor [B][SENSOR_LEN] (`sensor_table(B, ...)`, an
        array or a device tensor, taken as it is), row b the measurement model of stream b; noise [B][DIST_LEN] or None: the tick's unit draws.  Call it AHEAD
        of tick() (or pack()) and unsense() with the same table behind it (behind post(), AHEAD of plant_step(), log(), disturb() and update_device()): in
        between the robot records hold what the sensors hand out (`sense_robot` is the mirror), the truth waits in `self.sensor_state()`.  A stream without
        a plan takes no sample; a stream with an invalid row is left alone, its mask in the result.  Accumulates `self.sensor_rec` [B][SENSOR_REC_LEN] (slots
        SENSOR_REC; `tick` is what its TICK_* name), initialised on first use, and leaves in `self.meas` [B][RB_LEN] the records the pack will read.  One
        launch, asynchronous on `stream`, capturable.  Returns the `sensor_info` tensor [B] (int32), valid once `stream` has run the launch."""
        import torch
        sensor = self._dev64(sensor, (self.B, SENSOR["LEN"]), "sensor", stream)
        if noise is not None:
            noise = self._dev64(noise, (self.B, DIST_LEN), "noise", stream)
        state = self.sensor_state(stream)
        if self.sensor_rec is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
                self.sensor_info = torch.zeros((self.B,), dtype=torch.int32, device=self.path.device)
                rec0 = np.zeros(SENSOR_REC["LEN"])
                rec0[[SENSOR_REC["MAX_DQ"], SENSOR_REC["MAX_DP"]]], rec0[[SENSOR_REC["TICK_DQ"], SENSOR_REC["JOINT_DQ"], SENSOR_REC["TICK_DP"]]] = -np.inf, -1.0
                self.sensor_rec = torch.as_tensor(rec0).to(self.path.device).repeat(self.B, 1).contiguous()
                self.meas = torch.full((self.B, RB["LEN"]), float("nan"), dtype=torch.float64, device=self.path.device)
        _lib.check(self.solver._lib.bmpc_stream_sense(self.solver._h, self.B, _ptr(self.robot), _ptr(self.state), _ptr(sensor), _ptr(state), _ptr(self.sensor_info),
                                                      _ptr(self.sensor_rec), None if noise is None else _ptr(noise), _ptr(self.meas), int(tick), self._stream(stream)),
                   "bmpc_stream_sense")
        self._sense_inputs = (sensor, noise)      # the launch is asynchronous: its inputs live until the next one replaces them
        return self.sensor_info

    def unsense(self, sensor, stream=None):
        """The way back from the samples to the true plants behind a tick (bmpc_stream_unsense; `truth_robot` is the mirror): where the sample of sense()
        differed from the truth, the true plant takes the step the post took on the sample, under the same planned jerk, or comes back as it was where the
        post exhausted the plan.  sensor: the table sense() was given.  One launch, asynchronous on `stream`, capturable."""
        sensor = self._dev64(sensor, (self.B, SENSOR["LEN"]), "sensor", stream)
        _lib.check(self.solver._lib.bmpc_stream_unsense(self.solver._h, self.B, _ptr(self.robot), _ptr(self.state), _ptr(sensor), _ptr(self.sensor_state(stream)),
                                                        self._stream(stream)), "bmpc_stream_unsense")
        self._unsense_input = sensor

    def observer_state(self, stream=None):
        """the observers' state on the device, [B][OBSERVER_STATE_LEN] (slots OBSERVER_STATE): the last posterior and the jerks that advance it; zeros (fresh:
        the first sample is taken as it is) on first use, then carried from launch to launch, so rollouts chain"""
        import torch
        if self.observer_state_ is None:
            lib = self.solver._lib
            assert (lib.bmpc_stream_observer_len(), lib.bmpc_stream_observer_state_len(), lib.bmpc_stream_observer_rec_len()) == (OBSERVER["LEN"], OBSERVER_STATE["LEN"], OBSERVER_REC["LEN"])
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
                self.observer_state_ = torch.zeros((self.B, OBSERVER_STATE["LEN"]), dtype=torch.float64, device=self.path.device)
        return self.observer_state_

    def observer_reset(self, stream=None):
        """Start the observers afresh: a state of zeros (no posterior) and an empty `self.observer_rec`.  A per-tick loop that is to leave what
        rollout(observer=) leaves calls it, and sensor_reset(), where that launch would start.  Nothing else resets the state: not a disturbance, not a
        re-plan, not a lost plan."""
        self.observer_state_ = self.observer_rec = self.observer_info = self.sample = None
        return self.observer_state(stream)

    def observe(self, sensor, observer, noise=None, tick=0, stream=None):
        """The sensors and the observers between the plants and the controller, the sample of one tick and the estimate made from it (bmpc_stream_observe): sense()
        with observer [B][OBSERVER_LEN] (`observer_table(B, ...)`, an array or a device tensor, taken as it is), row b the state estimator of stream b, between
        the sample and the robot records.  Call it IN THE PLACE of sense(), ahead of tick() (or pack()), and unsense() with the same sensor table behind the
        tick: in between the robot records hold the estimates (`observe_robot` is the mirror and the specification), the truth waits in
        `self.sensor_state()`.  A stream without a plan takes no sample and makes no estimate; a stream with an invalid sensor or observer row is left alone,
        its masks in `self.sensor_info` and the result.  Accumulates `self.sensor_rec` (the samples against the truth) and `self.observer_rec`
        [B][OBSERVER_REC_LEN] (the estimates against the truth; slots OBSERVER_REC), initialised on first use, and leaves in `self.meas` [B][RB_LEN] the records
        the pack will read and in `self.sample` [B][DIST_LEN] the raw samples.  One launch, asynchronous on `stream`, capturable.  Returns the `observer_info`
        tensor [B] (int32), valid once `stream` has run the launch."""
        import torch
        sensor = self._dev64(sensor, (self.B, SENSOR["LEN"]), "sensor", stream)
        observer = self._dev64(observer, (self.B, OBSERVER["LEN"]), "observer", stream)
        if noise is not None:
            noise = self._dev64(noise, (self.B, DIST_LEN), "noise", stream)
        state, ostate = self.sensor_state(stream), self.observer_state(stream)
        dev = self.path.device
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(dev)):
            if self.sensor_rec is None:
                self.sensor_info = torch.zeros((self.B,), dtype=torch.int32, device=dev)
                rec0 = np.zeros(SENSOR_REC["LEN"])
                rec0[[SENSOR_REC["MAX_DQ"], SENSOR_REC["MAX_DP"]]], rec0[[SENSOR_REC["TICK_DQ"], SENSOR_REC["JOINT_DQ"], SENSOR_REC["TICK_DP"]]] = -np.inf, -1.0
                self.sensor_rec = torch.as_tensor(rec0).to(dev).repeat(self.B, 1).contiguous()
                self.meas = torch.full((self.B, RB["LEN"]), float("nan"), dtype=torch.float64, device=dev)
            if self.observer_rec is None:
                self.observer_info = torch.zeros((self.B,), dtype=torch.int32, device=dev)
                rec0 = np.zeros(OBSERVER_REC["LEN"])
                rec0[[OBSERVER_REC["MAX_DQ"], OBSERVER_REC["MAX_DP"]]], rec0[[OBSERVER_REC["TICK_DQ"], OBSERVER_REC["JOINT_DQ"], OBSERVER_REC["TICK_DP"]]] = -np.inf, -1.0
                self.observer_rec = torch.as_tensor(rec0).to(dev).repeat(self.B, 1).contiguous()
                self.sample = torch.full((self.B, DIST_LEN), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(self.solver._lib.bmpc_stream_observe(self.solver._h, self.B, _ptr(self.robot), _ptr(self.state), _ptr(sensor), _ptr(state), _ptr(self.sensor_info),
                                                        _ptr(self.sensor_rec), None if noise is None else _ptr(noise), _ptr(self.meas), int(tick), _ptr(observer), _ptr(ostate),
                                                        _ptr(self.observer_info), _ptr(self.observer_rec), _ptr(self.sample), self._stream(stream)), "bmpc_stream_observe")
        self._observe_inputs = (sensor, observer, noise)      # the launch is asynchronous: its inputs live until the next one replaces them
        return self.observer_info

    def _dev64(self, a, shape, name, stream, dtype=None):
        """`a` as a contiguous device tensor of `shape` (float64 unless dtype), copied on `stream` when it is not one already"""
        import torch
        dtype = dtype or torch.float64
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.ascontiguousarray(a))
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name} must be {list(shape)}, got {list(a.shape)}")
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.path.device)):
            return a.to(device=self.path.device, dtype=dtype).contiguous()

    def set_robot(self, rec):
        import torch
        self.robot.copy_(torch.as_tensor(np.ascontiguousarray(rec), dtype=torch.float64))

    def _stream(self, stream):
        return _stream_ptr(stream, self.path.device)

    @staticmethod
    def _flags(simulate, accept_capped):
        return int(bool(simulate)) | (2 if accept_capped else 0)

    def _tick_args(self, max_iter, warm_dual, simulate, accept_capped):
        """the arguments bmpc_stream_tick and bmpc_stream_graph_create share: everything between the handle and the stream / the graph"""
        return (self.B, _ptr(self.path), self.entries, _ptr(self.state), _ptr(self.robot), _ptr(self.p), _ptr(self.x0), _ptr(self.dual) if warm_dual else None,
                int(max_iter), _ptr(self.x), _ptr(self.g), _ptr(self.iters), _ptr(self.status), _ptr(self.kkt), _ptr(self.traj), self._flags(simulate, accept_capped))

    def pack(self, warm_dual=False, stream=None, continue_rejected=False):
        """continue_rejected (real-time mode): the warm start continues from the solver's last iterate when the acceptance rule rejected
        it (bmpc_stream_pack_rt with xlast = x), as the fused tick does; False = restart from the last accepted plan (the reference)."""
        _lib.check(self.solver._lib.bmpc_stream_pack_rt(self.solver._h, self.B, _ptr(self.path), self.entries, _ptr(self.state), _ptr(self.robot), _ptr(self.p),
                                                        _ptr(self.x0), _ptr(self.dual) if warm_dual else None, _ptr(self.x) if continue_rejected else None,
                                                        self._stream(stream)), "bmpc_stream_pack_rt")

    def post(self, simulate=True, stream=None, accept_capped=False):
        _lib.check(self.solver._lib.bmpc_stream_post(self.solver._h, self.B, _ptr(self.path), self.entries, _ptr(self.state), _ptr(self.robot), _ptr(self.x),
                                                     _ptr(self.g), _ptr(self.status), _ptr(self.traj), self._flags(simulate, accept_capped),
                                                     self._stream(stream)), "bmpc_stream_post")

    def log(self, stream=None):
        """The logging records of the plans the last tick left behind (bmpc_stream_log): the tensor [B][log_len(N)], rows for `unpack_log`.
        Call it after post(), tick() or tick_graph() and before the next pack; asynchronous on `stream` like them.  A stream without a plan
        has n_valid = 0 and a NaN body.  The buffer is allocated on first use and reused."""
        if self._log is None:
            import torch
            n = self.solver._lib.bmpc_stream_log_len(self.solver._h)
            assert n == log_len(self.N)
            self._log = torch.empty((self.B, n), dtype=torch.float64, device=self.path.device)
        _lib.check(self.solver._lib.bmpc_stream_log(self.solver._h, self.B, _ptr(self.path), self.entries, _ptr(self.state), _ptr(self.p), _ptr(self.traj),
                                                    _ptr(self._log), self._stream(stream)), "bmpc_stream_log")
        return self._log

    def tube(self, stream=None):
        """The tube and joint-limit excess of the measured state in `self.p` (bmpc_stream_tube): the tensor [B][tube_len()], slots TUBE -- what
        `tube_excess_of_state(self.p)` computes on the host, without the copy.  Call it behind pack(), tick() or tick_graph() and before the next
        pack; behind a tick it measures the state that tick started from.  A stream without a plan has a NaN row.  Asynchronous on `stream`; the
        buffer is allocated on first use and reused."""
        if self._tube is None:
            import torch
            assert self.solver._lib.bmpc_stream_tube_len() == TUBE["LEN"]
            self._tube = torch.empty((self.B, TUBE["LEN"]), dtype=torch.float64, device=self.path.device)
        _lib.check(self.solver._lib.bmpc_stream_tube(self.solver._h, self.B, _ptr(self.p), _ptr(self.state), _ptr(self._tube), self._stream(stream)), "bmpc_stream_tube")
        return self._tube

    def tick(self, max_iter=0, warm_dual=False, simulate=True, stream=None, accept_capped=False, fused=True):
        """pack -> solve -> post of one tick: one fused launch (bmpc_stream_tick; N <= 11, B within the resident waves) or, with
        fused=False, the three launches of the separate entry points (see tick_graph for the captured form).
        accept_capped: real-time mode -- an iteration-capped iterate is judged by the reference's violation rule with the handle's
        real-time threshold (BatchedOCPSolver.set_rt_feasibility_tol) and replaced by the previous plan if it fails."""
        if max_iter and not warm_dual:
            raise ValueError("an iteration cap needs the dual state (warm_dual=True): the multipliers must be shifted with the plan")
        if fused:
            _lib.check(self.solver._lib.bmpc_stream_tick(self.solver._h, *self._tick_args(max_iter, warm_dual, simulate, accept_capped), self._stream(stream)),
                       "bmpc_stream_tick")
            return
        self.pack(warm_dual, stream, continue_rejected=accept_capped)      # the same continuation rule as the fused launch
        out = dict(x=self.x, g=self.g, iters=self.iters, status=self.status, kkt=self.kkt)
        self.solver.solve_batch(self.p, self.x0, out=out, want=("g", "iters", "status", "kkt"), stream=stream,
                                state=self.dual if warm_dual else None, max_iter=max_iter)
        self.post(simulate, stream, accept_capped)

    def tick_with_fallback(self, fallback, max_iter=24, simulate=True, stream=None):
        """A tick of the converged loops with a barrier-level fallback (round 5): pack -> solve to tolerance with at most `max_iter` iterations (dual state
        carried) -> the streams whose solve did not converge are solved AGAIN from the same warm start by `fallback`, a handle on a fixed barrier level
        (BatchedOCPSolver(fixed_barrier=1.0, max_iter=14, ...)): a dozen Newton steps on a smooth barrier problem, far from the tube walls -> post, where
        the reference's acceptance rule (BoundMPC.py:460-465: solver success or summed violation below the handle's threshold, set it to the reference's 1e-4)
        decides for every stream.  What the converged loops lose their plans on are ticks whose minimiser cannot be reached (or does not exist) from the
        shifted plan; a plan of the level-1 problem is still a feasible trajectory, and the next tick usually converges again (CPU replay, 256 streams:
        14 lose their plan instead of 33; the restoration phase: 17-19, at three times the tick).  The fallback streams restart their dual state cold.
        Not captured in a graph: the count of failed streams is read on the host."""
        import torch
        N57 = self.N * 57
        self.pack(True, stream)
        dual0 = self.dual.clone()
        out = dict(x=self.x, g=self.g, iters=self.iters, status=self.status, kkt=self.kkt)
        self.solver.solve_batch(self.p, self.x0, out=out, want=("g", "iters", "status", "kkt"), stream=stream, state=self.dual, max_iter=max_iter)
        idx = torch.nonzero(self.status != 0).flatten()
        if idx.numel():
            st = dual0[idx].contiguous(); st[:, N57].clamp_(min=1e-9)      # warm: the multipliers of the shifted plan bound the initial slacks
            o = fallback.solve_batch(self.p[idx].contiguous(), self.x0[idx].contiguous(), want=("g", "iters", "status", "kkt"), stream=stream, state=st)
            self.x[idx] = o["x"]; self.g[idx] = o["g"]; self.iters[idx] += o["iters"]; self.kkt[idx] = o["kkt"]
            self.status[idx] = torch.where(o["status"] == 0, torch.ones_like(o["status"]), o["status"])      # a level plan is never "converged": the rule decides
            self.dual[idx] = 0.0
        self.post(simulate, stream, accept_capped=True)
        return int(idx.numel())

    def tick_graph(self, max_iter=0, warm_dual=False, simulate=True, stream=None, accept_capped=False):
        """The same tick replayed from a hipGraph captured on first use (bmpc_stream_graph_create)."""
        key = (int(max_iter), bool(warm_dual), bool(simulate), bool(accept_capped))
        if key not in self._graphs:
            if max_iter and not warm_dual:
                raise ValueError("an iteration cap needs the dual state (warm_dual=True)")
            g = ctypes.c_void_p()
            _lib.check(self.solver._lib.bmpc_stream_graph_create(self.solver._h, *self._tick_args(max_iter, warm_dual, simulate, accept_capped), ctypes.byref(g)),
                       "bmpc_stream_graph_create")
            self._graphs[key] = g
        # (a replay requested on the legacy null stream is run by the library on a stream of the handle, bracketed by events:
        # bmpc_graph_launch)
        _lib.check(self.solver._lib.bmpc_graph_launch(self._graphs[key], self._stream(stream)), "bmpc_graph_launch")

    def rollout(self, ticks, max_iter=0, warm_dual=False, accept_capped=False, goal_tol=0.0, want_traj=False, stream=None,
                replan=None, replan_tick=None, splice=True, poor_bounds=False, set_goal=True, disturb=None, audit=False, audit_tol=1e-6, want_tube=False,
                want_log=False, log_stages=1, track=False, waves=None, legs=None, leg_tick=None, leg_on=None, leg_tol=None, tune=None, want_tune_used=False,
                plant=None, want_plant_rec=False, sensor=None, sensor_noise=None, want_meas=False, want_sensor_rec=False, observer=None, want_sample=False,
                want_observer_rec=False):
        """`ticks` closed-loop ticks (plant simulation on) of every stream in ONE launch (bmpc_stream_rollout): each stream runs at its own pace, so
        the launch lasts as long as the slowest stream's SUM of solves, where a loop of tick() / tick_graph() pays the slowest stream of every tick.
        For closed loops run in bulk -- whole-loop throughput, any B; where a host reads or acts between ticks (a real plant, a time
        budget) use the ticks.  Waves per stream: the solver's set_rollout_waves (set_team_waves does not apply) -- 1, the default, one wave per
        stream; 4 a team of cooperating waves per stream whatever B is, striding over the resident teams (N <= 10, S <= 4; what pays up to 256 streams,
        where one wave per stream leaves three SIMDs of four idle); 0 teams when B fits into the resident teams, else one wave.  waves=None takes that
        setting; another value is set for this launch and the former one put back behind it (read at launch time: the launch stays asynchronous).  On
        teams "one wave per stream" below reads "a team per stream": the ticks of set_team_waves(4).  A stream stops once it has lost its plan (status 3, as
        the fused tick leaves a skipped stream) or, with goal_tol > 0, behind the tick that leaves phi_max - phi <= goal_tol (NodeLoop.run's rule).
        With goal_tol = 0 the batch's buffers hold afterwards what `ticks` calls of tick(fused=True) on one wave per stream leave, bit for bit.
        The protocol of closed_loop -- tick 0 solved out with first_cap, later ticks capped -- is
            sb.tick(first_cap, warm_dual=True); sb.rollout(T - 1, cap, warm_dual=True, accept_capped=...)
        Returns device tensors, valid once `stream` has run the launch (asynchronous, no synchronisation):
          hist [ticks][B][rollout_len()]   the history row of stream b behind tick t (slots ROLL, unpack_rollout); NaN for a tick it did not run
          ticks_run [B] int32              ticks the stream ran
          traj_hist [ticks][B][tr_len]     want_traj: the trajectory record of every tick (unpack_traj); NaN likewise
        EVENTS behind a tick's post (bmpc_stream_rollout_events; with replan, replan_tick and disturb all None the plain rollout runs):
          disturb [ticks][B][DIST_LEN]     row [t][b] disturbs the plant of stream b behind tick t (as disturb()); hist[t][b] shows the plant before it
          replan [B][replan_len], replan_tick [B]   the record of stream b (`replan_record`; `self.replan` itself is taken as it is) is consumed behind
                                           tick replan_tick[b] as update_device(set_goal, splice, poor_bounds) consumes it; splice (default here: the
                                           state behind that tick exists on the device only) writes the measured state into the record first.
        The goal test and the next tick's lost-plan test see what the re-plan left: a second leg starts behind the tick that reaches the old goal, a
        re-plan behind the post that exhausted the plan rescues the stream.  A stream that stops before its tick keeps its record's flag raised.
        Then the result also holds  replan_info [B] int32: -1 not consumed, 0 consumed, 1 invalid record.
        AUDIT behind a tick's pack (bmpc_stream_rollout_audit; with audit and want_tube both off the entries above run unchanged):
          want_tube: tube_hist [ticks][B][tube_len()]   row [t][b] (slots TUBE) measures the state tick t of stream b STARTS from -- the plant behind
                                           tick t - 1 with its disturbance and re-plan applied, what tube() behind tick t returns; NaN likewise
          audit: audit [B][12]             the stream's verdict over its rows (slots AUDIT, unpack_audit): largest excesses and their ticks, samples
                                           outside by more than audit_tol, joint-limit samples, the first tick outside a tube.
        LOG behind a tick's post, ahead of its events (bmpc_stream_rollout_log; with want_log and track both off the entries above run unchanged):
          want_log: log_hist [ticks][B][rollout_log_len(log_stages)]   row [t][b] holds the first log_stages (1..N) stages of what log() returns
                                           behind tick t -- path reference, tube bounds, errors in the path frame (unpack_log(row, N, log_stages)) --
                                           with the n_valid of the whole plan; NaN likewise
          track: track [B][12]             the stream's tracking record over stage 0 of its rows, the state the plant is in behind every tick (slots
                                           TRACK, unpack_track): largest ||e_p_orth||, ||e_p_par||, ||e_r|| with their ticks, sums of squares, replays.
        MISSIONS (bmpc_stream_rollout_legs; exclusive with replan / replan_tick; without `legs` nothing changes): a QUEUE of K re-plan records per stream
        in the place of the one scheduled record -- task sequences and recovery policies in one launch, every stream at its own pace.
          legs [B][K][replan_len]          records (tensor or array), or B lists of K `replan_record`s; copied into a device buffer kept in `self.legs`
                                           (passing `self.legs` itself copies nothing); consumed as replan is: set_goal, splice, poor_bounds
          leg_tick [B][K] int              record k is due at or after this tick; negative (the default for all): no tick condition
          leg_on [B][K] int                LEG["AT_GOAL"]: due once phi_max - phi <= its tolerance; LEG["ON_LOST"]: due when the post of a tick
                                           exhausted the plan; default 0.  A record without any condition (or with an unknown bit) ends the queue.
          leg_tol [B][K]                   the goal tolerance of record k; None: goal_tol for every record
        Only the head of a stream's queue can fire, one record per tick, where the single re-plan sits: a goal-triggered record gives the stream its next
        phi_max before the goal test sees the old one (with goal_tol > 0 a stream stops only at the goal of its last leg), an on-lost record rescues it.
        Then the result also holds  legs_done [B] int32: records consumed;  leg_fired [B][K]: the tick behind which record k was consumed, -1 never;
        leg_why [B][K]: LEG["WHY_GOAL"] | LEG["WHY_LOST"] | LEG["WHY_TICK"], 0 never;  replan_info [B][K]: -1 not consumed, 0 consumed, 1 invalid.
        The audit and the tracking record run over the whole mission; per-leg spans follow from leg_fired.
        SWEEPS (bmpc_stream_rollout_tuned; with or without `legs`, not with replan / replan_tick; without `tune` nothing changes): controller settings
        per stream in the place of the one set the handle carries -- a grid over settings is one launch of as many streams, not as many handles.
          tune [B][TUNE_LEN]               `tune_table(B, ...)`, an array or a device tensor (taken as it is): row b, slots TUNE, replaces for every
                                           tick of stream b the iteration cap, tol, the barrier start and hold, the level rule, the acceptance threshold
                                           and position-row cap, bound_margin and the stall window; a NaN slot keeps the handle's value as this launch
                                           reads it (MAX_ITER: the max_iter argument when > 0).  An iteration cap in the table needs warm_dual as well.
        The rows are validated on the device.  A row with an invalid slot does not run: ticks_run 0, NaN rows, untouched tick arrays, and
          tune_info [B] int32              0: the row was valid and the stream ran; else the bit mask of its invalid slots (bit TUNE_CROSS: the level
                                           rule as resolved) -- READ IT: the other streams are served as if the row were not there
          tune_used [B][TUNE_LEN]          want_tune_used: the rows as resolved (unpack_tune), what the streams ran with or were refused for.
        Every array of stream b holds what the same call without a table leaves for the one-stream batch {b} on a solver set up from tune_used[b].
        PLANTS (bmpc_stream_rollout_plant; with or without `legs` and `tune`, not with replan / replan_tick; without `plant` nothing changes): an actuator
        model per stream between the first planned jerk of every tick and the plant, which otherwise IS the model -- "gain error x lag x margin" is one
        launch whose audit answers.
          plant [B][PLANT_LEN]             `plant_table(B, gain=, bias=, lag=, sat=, delay=)`, an array or a device tensor (taken as it is): row b, slots
                                           PLANT; a NaN slot is the identity.  The step (`plant_robot` is the mirror) sits behind the post of every tick that
                                           stepped the plant, AHEAD of that tick's rows, disturbance and re-plan: hist[t][b] shows the TRUE plant, the next
                                           pack and tube_hist[t + 1][b] / audit measure it.  log_hist and track keep describing the PLAN, not the plant.
        The drives' state is `self.plant_state` [B][PLANT_STATE_LEN], created from the robot records on first use (plant_state_of) and carried from launch to
        launch, so rollouts chain.  The rows are validated on the device; a row with an invalid slot does not run, as an invalid tune row.
          plant_info [B] int32             0: the row was valid and the stream ran; else the bit mask of its invalid slots -- READ IT
          plant_rec [B][PLANT_REC_LEN]     want_plant_rec: what the drives did to the commands (slots PLANT_REC, unpack_plant_rec).
        SENSORS (bmpc_stream_rollout_sensor; with or without `legs`, `tune` and `plant`, not with replan / replan_tick; without `sensor` nothing changes): a
        measurement model per stream between the plant and what the pack, the solve and the post of every tick read, which otherwise IS the plant --
        "encoder resolution x lag x margin" is one launch.
          sensor [B][SENSOR_LEN]           `sensor_table(B, bias=, res=, nq=, ndq=, nddq=, hold=)`, an array or a device tensor (taken as it is): row b,
                                           slots SENSOR; a NaN slot is the identity.  The sample (`sense_robot` is the mirror) is taken ahead of every pack,
                                           the way back to the truth (`truth_robot`) sits behind the post, ahead of the plant step.
          sensor_noise [ticks][B][DIST_LEN]   unit draws made by the caller, scaled by the row's NQ, NDQ, NDDQ; None: zeros
        WHAT EACH OUTPUT THEN DESCRIBES.  hist, `self.robot` behind the launch, what disturb acts on, what the plant step corrects, what a spliced re-plan
        takes and what the next launch starts from: the TRUTH.  `self.p`, tube_hist and audit (taken from the pack's p), traj_hist, log_hist and track: the
        MEASUREMENT and the plan made from it -- what the controller's own monitor would report.
          meas_hist [ticks][B][RB_LEN]     want_meas: the robot record the pack of tick t read; NaN for a tick the stream did not run
          sensor_info [B] int32            0: the row was valid and the stream ran; else the bit mask of its invalid slots -- READ IT
          sensor_rec [B][SENSOR_REC_LEN]   want_sensor_rec: what the samples differed from the truth by (slots SENSOR_REC, unpack_sensor_rec); its max_dp
                                           bounds what the audit's position excess can miss.
        The sensors' state is `self.sensor_state()` [B][SENSOR_STATE_LEN], zeros on first use and carried from launch to launch, so rollouts chain.
        OBSERVERS (bmpc_stream_rollout_observer; with `sensor` only; without `observer` nothing changes): a state estimator per stream between the sensor's
        sample and what the pack, the solve and the post of every tick read, which otherwise IS the noisy sample -- "encoder resolution x lag x margin x
        filter" is one launch.
          observer [B][OBSERVER_LEN]       `observer_table(B, lq=, ldq=, lddq=, lead=, gate=)`, an array or a device tensor (taken as it is): row b, slots
                                           OBSERVER; a NaN slot is the identity.  A predictor-corrector on the model's own jerk-integrator chain
                                           (`observe_robot` is the mirror and the specification): gains on q, dq, ddq, one step of lead for a sample that is
                                           one tick old (the sensor's HOLD), an innovation gate.  The estimate is installed where the sample is.
          meas_hist                        keeps its meaning, the record the pack of tick t read: it is now the ESTIMATE's record
          sensor_rec                       keeps its meaning: the samples against the truth
          sample_hist [ticks][B][DIST_LEN]   want_sample: the raw sample of tick t; NaN for a tick the stream did not run
          observer_info [B] int32          0: the row was valid and the stream ran; else the bit mask of its invalid slots -- READ IT
          observer_rec [B][OBSERVER_REC_LEN]   want_observer_rec: what the estimates differed from the truth by and how many samples the gate rejected
                                           (slots OBSERVER_REC, unpack_observer_rec)
        The observers' state is `self.observer_state()` [B][OBSERVER_STATE_LEN], zeros on first use and carried from launch to launch, so rollouts chain.  The
        observer is not told of a disturbance, a spliced re-plan or a post that exhausted the plan: its prediction is then off, the innovation pulls it back
        as a real filter's would, and the state is not reset."""
        import torch
        former = self.solver.rollout_waves
        if waves is not None:
            self.solver.set_rollout_waves(waves)      # (a refused value raises here, the setting intact)
        try:
            # 1. the argument checks
            scheduled = replan is not None or replan_tick is not None
            if max_iter and not warm_dual:
                raise ValueError("an iteration cap needs the dual state (warm_dual=True): the multipliers must be shifted with the plan")
            if want_log and not 1 <= int(log_stages) <= self.N:
                raise ValueError("log_stages must be in 1..N")
            if tune is not None and scheduled:
                raise ValueError("tune goes with legs, the queue of re-plan records: it does not go with replan / replan_tick")
            if tune is None and want_tune_used:
                raise ValueError("want_tune_used goes with tune")
            if plant is None and want_plant_rec:
                raise ValueError("want_plant_rec goes with plant")
            if plant is not None and scheduled:
                raise ValueError("plant goes with legs, the queue of re-plan records: it does not go with replan / replan_tick")
            if sensor is None and (sensor_noise is not None or want_meas or want_sensor_rec):
                raise ValueError("sensor_noise, want_meas and want_sensor_rec go with sensor")
            if sensor is not None and scheduled:
                raise ValueError("sensor goes with legs, the queue of re-plan records: it does not go with replan / replan_tick")
            if observer is None and (want_sample or want_observer_rec):
                raise ValueError("want_sample and want_observer_rec go with observer")
            if observer is not None and sensor is None:
                raise ValueError("observer goes with sensor: there is no sample to filter without one")
            if legs is not None and scheduled:
                raise ValueError("legs is the queue of re-plan records: it does not go with replan / replan_tick")
            if legs is None and (leg_tick is not None or leg_on is not None or leg_tol is not None):
                raise ValueError("leg_tick, leg_on and leg_tol describe the records of legs")
            if (replan is None) != (replan_tick is None):
                raise ValueError("replan and replan_tick go together")
            name = rollout_entry(replan=replan is not None, replan_tick=replan_tick is not None, disturb=disturb is not None, audit=bool(audit), want_tube=bool(want_tube),
                                 want_log=bool(want_log), track=bool(track), legs=legs is not None, tune=tune is not None, plant=plant is not None)
            entry = ROLLOUT_ENTRIES.index(name)
            if sensor is not None:      # (the sensor's entry, chosen here: it takes every group of the plants' entry and the sensor's behind them)
                name, entry = "bmpc_stream_rollout_sensor", len(ROLLOUT_ENTRIES)
            if observer is not None:      # (the observer's entry: the groups of the sensor's entry and the observer's behind them)
                name, entry = "bmpc_stream_rollout_observer", len(ROLLOUT_ENTRIES) + 1
            flags = self._update_flags(set_goal, splice, poor_bounds) if entry else 0      # (the plain rollout has no events: their words are not looked at)
            lib, B, n, dev = self.solver._lib, self.B, max(int(ticks), 0), self.path.device
            assert lib.bmpc_stream_rollout_len() == ROLL["LEN"] and (not track or lib.bmpc_stream_track_len() == TRACK["LEN"]) and (tune is None or lib.bmpc_stream_tune_len() == TUNE["LEN"])
            assert not want_log or lib.bmpc_stream_rollout_log_len(self.solver._h, int(log_stages)) == rollout_log_len(log_stages)
            # 2. every input on the device, once
            record = state = sstate = ostate = None
            K = 0
            if replan is not None:
                record = self._replan_buffer(replan, stream)
                replan_tick = self._dev64(replan_tick, (B,), "replan_tick", stream, dtype=torch.int32)
            if legs is not None:
                K = self._legs_buffer(legs, stream)
                record = self.legs
                i32 = lambda a, fill, what: torch.full((B, K), fill, dtype=torch.int32, device=dev) if a is None else self._dev64(a, (B, K), what, stream, dtype=torch.int32)
                leg_tick, leg_on = i32(leg_tick, -1, "leg_tick"), i32(leg_on, 0, "leg_on")
                if leg_tol is not None:
                    leg_tol = self._dev64(leg_tol, (B, K), "leg_tol", stream)
            if disturb is not None:
                disturb = self._dev64(disturb, (n, B, DIST_LEN), "disturb", stream)
            if tune is not None:
                tune = self._dev64(tune, (B, TUNE["LEN"]), "tune", stream)
            if plant is not None:
                plant, state = self._dev64(plant, (B, PLANT["LEN"]), "plant", stream), self._plant_state(stream)
            if sensor is not None:
                assert lib.bmpc_stream_sensor_len() == SENSOR["LEN"]
                sensor, sstate = self._dev64(sensor, (B, SENSOR["LEN"]), "sensor", stream), self.sensor_state(stream)
                if sensor_noise is not None:
                    sensor_noise = self._dev64(sensor_noise, (n, B, DIST_LEN), "sensor_noise", stream)
            if observer is not None:
                assert lib.bmpc_stream_observer_len() == OBSERVER["LEN"]
                observer, ostate = self._dev64(observer, (B, OBSERVER["LEN"]), "observer", stream), self.observer_state(stream)
            # 3. every output, once
            out = {"hist": torch.empty((n, B, ROLL["LEN"]), dtype=torch.float64, device=dev), "ticks_run": torch.zeros((B,), dtype=torch.int32, device=dev)}
            for key, want, shape in (("traj_hist", want_traj, (n, B, self.tr_len)), ("audit", audit, (B, AUDIT["LEN"])), ("tube_hist", want_tube, (n, B, TUBE["LEN"])),
                                     ("log_hist", want_log, (n, B, rollout_log_len(log_stages) if want_log else 0)), ("track", track, (B, TRACK["LEN"])),
                                     ("tune_used", want_tune_used, (B, TUNE["LEN"])), ("plant_rec", want_plant_rec, (B, PLANT_REC["LEN"])),
                                     ("meas_hist", want_meas, (n, B, RB["LEN"])), ("sensor_rec", want_sensor_rec, (B, SENSOR_REC["LEN"])),
                                     ("sample_hist", want_sample, (n, B, DIST_LEN)), ("observer_rec", want_observer_rec, (B, OBSERVER_REC["LEN"]))):
                if want:
                    out[key] = torch.empty(shape, dtype=torch.float64, device=dev)
            for key, want, shape, fill in (("tune_info", tune is not None, (B,), -1), ("plant_info", plant is not None, (B,), -1), ("sensor_info", sensor is not None, (B,), -1), ("observer_info", observer is not None, (B,), -1), ("legs_done", K, (B,), 0), ("leg_fired", K, (B, K), -1),
                                           ("leg_why", K, (B, K), 0), ("replan_info", K or 1 <= entry <= 3, (B, K) if K else (B,), -1)):
                if want:
                    out[key] = torch.full(shape, fill, dtype=torch.int32, device=dev)
            # 4. the argument tuple of the entry: the common prefix, then the groups its signature states -- entry k takes the first k of them
            at = lambda t: None if t is None else _ptr(t)
            o = lambda key: at(out.get(key))
            tick = self._tick_args(max_iter, warm_dual, True, accept_capped)
            prefix = (self.solver._h, tick[0], int(ticks), *tick[1:], float(goal_tol), o("hist"), o("traj_hist"), o("ticks_run"))
            groups = ((at(record),) + ((at(replan_tick),) if entry <= 3 else ()) + (o("replan_info"), flags, at(disturb)),      # events: the scheduled record (1 to 3) or the queue's
                      (o("tube_hist"), o("audit"), float(audit_tol)),                                                          # audit
                      (o("log_hist"), int(log_stages), o("track")),                                                            # log
                      (K, at(leg_tick), at(leg_on), at(leg_tol), o("legs_done"), o("leg_fired"), o("leg_why")),                 # queue
                      (at(tune), o("tune_info"), o("tune_used")),                                                              # table
                      (at(plant), at(state), o("plant_info"), o("plant_rec")),                                                 # plant
                      (at(sensor), at(sstate), o("sensor_info"), o("sensor_rec"), at(sensor_noise), o("meas_hist")),             # sensor
                      (at(observer), at(ostate), o("observer_info"), o("observer_rec"), o("sample_hist")))                        # observer
            _lib.check(getattr(lib, name)(*prefix, *(a for group in groups[:entry] for a in group), self._stream(stream)), name)
            if entry:
                self._event_inputs = (replan_tick, leg_tick, leg_on, leg_tol, disturb, tune, plant, sensor, sensor_noise, observer)      # the launch is asynchronous: its inputs live until the next one replaces them
            return out
        finally:
            if waves is not None:
                self.solver.set_rollout_waves(former)

    def closed_loop(self, ticks, cap=0, warm=True, accept_capped=False, first_cap=100, budget_us=None, graph=True, fused=True, timed=False, tick=None):
        """THE closed loop of BASELINE configs[4], as a generator over the tick index: `for t in sb.closed_loop(ticks, ...)`.
        Tick 0 is every stream's cold start from rest, solved out (`first_cap` iterations, dual state kept, the reference's acceptance rule,
        no time budget); warm=False zeroes the dual state behind it (cold duals on every tick).  Later ticks run at most `cap` iterations
        (0 = the handle's) under the real-time acceptance rule if accept_capped.  What runs on a later tick:
          tick=f        f(), a caller's own tick body (graph is not looked at);
          graph=True    the replay of the captured graph;
          graph=False   a direct launch of self.tick.
        fused is passed on to every self.tick the driver calls, tick 0 included (False: the three-kernel tick); a graph is always the fused tick.
        budget_us: time budget of the fused ticks after the first (the handle's setting is read at capture: off for tick 0, set behind it).
        timed=True: HIP events around every tick after the first, `self.tick_ms` holds the time of the tick just run (None for tick 0).  The
        launch stream has been synchronised when the loop body runs; what to record there is the caller's business.
        Where nothing is read between the ticks, the same protocol in two launches is tick(first_cap, warm_dual=True) + rollout(ticks - 1, cap, ...)."""
        import torch
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)] if timed else None
        for t in range(ticks):
            self.tick_ms = None
            if t == 0:
                if budget_us is not None:
                    self.solver.set_time_budget_us(0)
                self.tick(max_iter=first_cap, warm_dual=True, simulate=True, fused=fused)
                if not warm:
                    self.dual.zero_()
                if budget_us is not None:
                    self.solver.set_time_budget_us(budget_us)
            else:
                if timed:
                    ev[0].record()
                if tick is not None:
                    tick()
                elif graph:
                    self.tick_graph(max_iter=cap, warm_dual=warm, simulate=True, accept_capped=accept_capped)
                else:
                    self.tick(max_iter=cap, warm_dual=warm, simulate=True, accept_capped=accept_capped, fused=fused)
                if timed:
                    ev[1].record(); ev[1].synchronize()
                    self.tick_ms = ev[0].elapsed_time(ev[1])
            if self.tick_ms is None:
                torch.cuda.current_stream(self.state.device).synchronize()
            yield t

    # the named reads (module functions above) on this batch's own buffers
    def applied(self):
        return applied(self.traj)

    def g_viol(self):
        return g_viol(self.traj)

    def has_plan(self):
        return has_plan(self.state, self.N)

    def valid(self):
        return valid(self.state)

    def phi(self):
        return phi(self.state)

    def level(self):
        return level(self.dual, self.N)

    def tick_tube_figures(self):
        return tick_tube_figures(self.p, self.state, self.g, self.traj, self.N, self.S)

    def close(self):
        for g in self._graphs.values():
            self.solver._lib.bmpc_graph_destroy(g)
        self._graphs = {}
        _give_start_rollout_back(self.solver, getattr(self, "_rollout_was", None))      # the handle's start-rollout setting as it was found
        self._rollout_was = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
