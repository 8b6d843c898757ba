"""TEST-ONLY: the CPU build of the stream re-planning and of the two event functions (boundmpc_amd/csrc/bmpc_stream_update.inl, bmpc_stream_events.inl
through tests/emu/bmpc_emu_stream_update.cpp) and what the CPU and the GPU tests of them share: random paths with the degenerate branches, and the comparison of a table / state pair."""
import ctypes

import numpy as np
from scipy.spatial.transform import Rotation as R

from boundmpc_amd import stream as bstream
from tests.emu import emu

PT, SS, RP, RV = bstream.PT, bstream.SS, bstream.RP, bstream.RV


def lib():
    L = emu._build("libbmpc_emu_stream_update.so", "bmpc_emu_stream_update.cpp", (), ("bmpc_stream.inl", "bmpc_stream_update.inl", "bmpc_stream_events.inl"))
    assert L.bmpc_emu_stream_disturb_len() == bstream.DIST_LEN
    return L


def stream_update(N, S, rec, path, ss, rb=None, set_goal=True):
    """One stream through the CPU build.  rec: re-plan record, path [cap][48], ss state row, rb robot record or None; nothing is modified.
    Returns (info, rec, path, ss, rb) after the call."""
    L = lib()
    rec, path, ss = (np.array(a, dtype=np.float64, order="C") for a in (rec, path, ss))
    rb = None if rb is None else np.array(rb, dtype=np.float64, order="C")
    cap = path.shape[0]
    assert path.shape[1] == PT["LEN"] and ss.shape == (bstream.ss_len(N),) and cap >= S + 1
    assert L.bmpc_emu_stream_replan_len(ctypes.c_int(S), ctypes.c_int(cap)) == bstream.replan_len(S, cap) == rec.shape[0]
    info = L.bmpc_emu_stream_update(ctypes.c_int(N), ctypes.c_int(S), emu._p(rec), emu._p(path), ctypes.c_int(cap), emu._p(ss), emu._p(rb), ctypes.c_int(int(bool(set_goal))))
    return info, rec, path, ss, rb


def stream_splice(h, S, rec, rb, poor_bounds=False, flags=None):
    """the CPU build of stream_splice on a copy of the record -> the record after it"""
    rec, rb = np.array(rec, dtype=np.float64, order="C"), np.array(rb, dtype=np.float64, order="C")
    cap = (rec.shape[0] - RP["HEAD"]) // RV["LEN"] + S - 1
    lib().bmpc_emu_stream_splice(ctypes.c_double(h), ctypes.c_int(S), ctypes.c_int(cap), emu._p(rec), emu._p(rb), ctypes.c_int(2 | (4 if poor_bounds else 0) if flags is None else flags))
    return rec


def stream_disturb(rb, d):
    """the CPU build of stream_disturb on a copy of the robot record -> the record after it"""
    rb, d = np.array(rb, dtype=np.float64, order="C"), np.array(d, dtype=np.float64, order="C")
    assert d.shape == (bstream.DIST_LEN,)
    lib().bmpc_emu_stream_disturb(emu._p(rb), emu._p(d))
    return rb


def stream_update_flags(N, S, h, rec, path, ss, rb, flags):
    """what bmpc_stream_update(flags) does with one stream, on copies -> (info, rec, path, ss, rb); info -2: the C ABI's BMPC_ERR_ARG"""
    rec, path, ss = (np.array(a, dtype=np.float64, order="C") for a in (rec, path, ss))
    rb = None if rb is None else np.array(rb, dtype=np.float64, order="C")
    info = lib().bmpc_emu_stream_update_flags(ctypes.c_int(N), ctypes.c_int(S), ctypes.c_double(h), emu._p(rec), emu._p(path), ctypes.c_int(path.shape[0]), emu._p(ss), emu._p(rb),
                                              ctypes.c_int(int(flags)))
    return info, rec, path, ss, rb


def random_path(rng, n, nb=None, vanish_first=False, vanish_later=False, no_rotation=False):
    """The arguments of apply_update after (ss, N, S) as a dict, for a random path of n via points: relative rotations of at most 2.5 rad, basis
    vectors well off their directions.  vanish_first: via point 1 coincides with via point 0 (with a rotation: the [0,1,0] direction and a
    pure-rotation length); vanish_later (n >= 3): the last via point coincides with the one before it, with a rotation (inherited direction,
    pure-rotation length); no_rotation: segment 0 has no rotation (the [0,1,0] axis fallback of unit_or_y)."""
    nb = n if nb is None else nb
    assert not (vanish_later and n < 3) and not (vanish_first and no_rotation)
    dP = [rng.uniform(0.05, 0.3) * _unit(rng.normal(size=3)) for _ in range(n - 1)]
    dR = [R.from_rotvec(rng.uniform(0.1, 2.5) * _unit(rng.normal(size=3))).as_matrix() for _ in range(n - 1)]
    if vanish_first:
        dP[0] = np.zeros(3)
    if vanish_later:
        dP[n - 2] = np.zeros(3)
    if no_rotation:
        dR[0] = np.eye(3)
    P, Rm = [rng.uniform(-0.5, 0.5, 3)], [R.from_rotvec(rng.uniform(0.2, 2.0) * _unit(rng.normal(size=3))).as_matrix()]
    for i in range(n - 1):
        P.append(P[-1] + dP[i]); Rm.append(dR[i] @ Rm[-1])
    lim = lambda lo, hi: [rng.uniform(lo, hi, 2) for _ in range(n)]
    return dict(pos_points=P, rot_points=Rm, pos_lim=[lim(-0.1, -0.01), lim(0.01, 0.1)], rot_lim=[lim(-0.3, -0.05), lim(0.05, 0.3)],
                bp1=[rng.normal(size=3) for _ in range(nb)], br1=[rng.normal(size=3) for _ in range(nb)],
                s=list(rng.uniform(0.1, 0.5, n)), e_p_min=list(rng.uniform(0.001, 0.01, n)), e_r_min=list(rng.uniform(0.01, 0.05, n)),
                e_p_max=list(rng.uniform(0.1, 0.5, n)), e_r_max=list(rng.uniform(0.2, 0.9, n)),
                p=P[0] + rng.normal(size=3) * 0.02, v=rng.normal(size=6) * 0.1, a=rng.normal(size=6) * 0.1, jerk=rng.normal(size=6) * 0.1,
                p0=np.concatenate([P[0] + rng.normal(size=3) * 0.02, rng.normal(size=3)]), weights=rng.uniform(0.1, 10.0, 15))


def _unit(v):
    return v / np.linalg.norm(v)


def args_of(path):
    """the dict of random_path (or one made by hand) in the argument order of apply_update after (ss, N, S)"""
    return [path[k] for k in ("pos_points", "rot_points", "pos_lim", "rot_lim", "bp1", "br1", "s", "e_p_min", "e_r_min", "e_p_max", "e_r_max", "p", "v", "a", "jerk",
                              "p0", "weights")]


def g11_args():
    """the re-planning fixture G11 recorded (upd_* of tests/golden/g11_update.npz) in the argument order of apply_update after (ss, N, S), as
    tests/test_stream.py test_stream_replanning_matches_reference_update_g11 passes it"""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "g11_update.npz"))
    L = lambda k: [np.array(v) for v in d["upd_" + k]]
    return [L("p_via"), L("r_via"), [L("p_lower"), L("p_upper")], [L("r_lower"), L("r_upper")], L("bp1"), L("br1"), list(d["upd_s"]), list(d["upd_e_p_min"]),
            list(d["upd_e_r_min"]), list(d["upd_e_p_max"]), list(d["upd_e_r_max"]), d["upd_p"], d["upd_v"], d["upd_a"], d["upd_jerk"], d["upd_p"], d["weights"]]


def random_state(rng, N, error_count=0, has_prev=False):
    """a state row with every word the re-planning must keep filled with noise"""
    ss = np.zeros(bstream.ss_len(N))
    ss[:SS["PREV"]] = rng.normal(size=SS["PREV"])
    ss[SS["SECTOR"]], ss[SS["HASPREV"]], ss[SS["ERRCNT"]] = 2, float(has_prev), error_count
    if has_prev:
        ss[SS["PREV"]:SS["PREV"] + 56 * N] = rng.normal(size=56 * N)
    return ss


def flip_pi(got, want):
    """`want` with the rotation vectors of angle pi turned onto the side of `got` (the flip rule of emu_stream_log.assert_equals_g10: a rotation vector of
    angle pi and its negative are the same rotation); got, want [..][3]"""
    got, want = np.asarray(got, dtype=float), np.array(want, dtype=float)
    flip = (np.abs(np.linalg.norm(want, axis=-1) - np.pi) < 1e-9) & (np.sum(got * want, axis=-1) < 0)
    want[flip] *= -1.0
    return want


def max_deviation(T, ss, T_ref, ss_ref):
    """largest absolute deviation of a table / state pair from another, PT_RRV and SS_PRREF under the flip rule; NaN where exactly one side is non-finite"""
    T_ref, ss_ref = np.array(T_ref, dtype=float), np.array(ss_ref, dtype=float)
    T_ref[:, PT["RRV"]:PT["RRV"] + 3] = flip_pi(T[:, PT["RRV"]:PT["RRV"] + 3], T_ref[:, PT["RRV"]:PT["RRV"] + 3])
    ss_ref[SS["PRREF"]:SS["PRREF"] + 3] = flip_pi(ss[SS["PRREF"]:SS["PRREF"] + 3], ss_ref[SS["PRREF"]:SS["PRREF"] + 3])
    worst = 0.0
    for a, b in ((T, T_ref), (ss, ss_ref)):
        fa, fb = np.isfinite(a), np.isfinite(b)
        if not np.array_equal(fa, fb):
            return float("nan")
        if fa.any():
            worst = max(worst, float(np.abs(a[fa] - b[fb]).max()))
    return worst


def assert_close(T, ss, T_ref, ss_ref, atol, what=""):
    """table (all rows) and state (the whole row) within atol of the other pair, the same entries non-finite on both sides"""
    dev = max_deviation(T, ss, T_ref, ss_ref)
    assert dev <= atol, f"{what}: deviation {dev} (nan: the non-finite entries differ)"
    return dev
