"""CPU: the tube measurement of the device (csrc/bmpc_stream_tube.inl, bmpc_stream_tube) and the rollout with the audit (bmpc_rollout_kernel.inl with AU,
bmpc_stream_rollout_audit) as g++ builds of their own text (tests/emu): the tube row against boundmpc_amd.stream.tube_excess_of_state and the joint
limits on the parameter vectors of the fixtures, hand-made rows, and the audit of an emulated rollout against the per-tick loop and the numpy reduction.
Tolerance of the rows against numpy: measured here on the CPU (profiles/stream_audit.txt: at most 3.6e-15 in any slot group), asserted at ten times that and
not below 1e-13 -- l and w are sums of a few O(1) products; the segment is compared exactly."""
import ctypes
import functools
import os

import numpy as np
import pytest

from boundmpc_amd import stream as bstream
from tests.emu import emu, emu_rollout as er, emu_stream_tube as et

TUBE, AUDIT, SS = bstream.TUBE, bstream.AUDIT, bstream.SS
ATOL = 1e-13
N, S, T, H = 2, 2, 6, 0.1
TOL = 1e-6


def _phi_sweep():
    """a g7 parameter vector with phi0 put into the middle of every window segment and beyond the last switch: every segment index of S = 4"""
    base, o = et.hand_made()["base"], bstream._poff(4)
    sw = base[o["sw"]:o["sw"] + 5]
    out = []
    for phi in [0.5 * (sw[i] + sw[i + 1]) for i in range(4)] + [sw[4] + 0.1, sw[0] - 0.05]:
        p = base.copy(); p[o["phi0"]] = phi
        out.append(p)
    return np.stack(out)


def test_slot_maps_and_lengths():
    L = et.lib()
    assert bstream.tube_len() == TUBE["LEN"] == L.bmpc_emu_stream_tube_len() == 16 and AUDIT["LEN"] == L.bmpc_emu_stream_audit_len() == 12
    assert sorted(v for k, v in TUBE.items() if k != "LEN") == [0, 5, 10, 11, 12, 13, 14, 15]
    assert sorted(v for k, v in AUDIT.items() if k != "LEN") == list(range(11))
    row = np.arange(12.0); row[AUDIT["FIRST_OUT"]] = -1.0
    u = bstream.unpack_audit(row)
    assert u["samples"] == 0 and u["max_pos"] == 1.0 and u["tick_pos"] == 2 and u["n_joint"] == 9 and u["first_out"] is None


def test_the_cpu_build_equals_numpy_on_the_fixtures():
    """every p of g7 exp1 / exp2, every stored p of g14 (orientation excess up to 0.13 rad and more), G9 at (10, 4) and at the shapes (3, 2), (5, 3), (4, 5),
    and a sweep of phi0 over the window of a g7 vector"""
    g9 = np.load(os.path.join(et.G, "g9_nlp.npz"))
    sets = {"g7": (10, 4, et.g7_p()), "g14": (10, 4, et.g14_p()), "g9 (10, 4)": (10, 4, g9["n10_p"]), "phi sweep": (10, 4, _phi_sweep())}
    sets.update({f"g9 {k}": (k[0], k[1], v) for k, v in et.g9_p().items()})
    worst, rot, segs = {}, [], set()
    for name, (n, s, p) in sets.items():
        got, want = et.stream_tube(n, s, p), et.numpy_rows(p, s)
        dev = et.deviations(got, want)
        print(f"{name:12s} {len(p):4d} vectors  " + "  ".join(f"{k} {v:.3e}" for k, v in dev.items()))
        for k, v in dev.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if s == 4:
            rot.append(want[:, TUBE["EX_ROT"]]); segs |= set(want[:, TUBE["SEG"]].astype(int).tolist())
    print("largest abs difference per slot group:", "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    rot = np.concatenate(rot)
    assert (rot > 1e-3).any() and (rot < 0).any() and segs == {0, 1, 2, 3}      # the inputs are not vacuous
    assert max(worst.values()) <= ATOL, worst


def test_hand_made_rows():
    """p0 moved 5 cm along bp1, a joint angle and a joint velocity beyond their limits, a NaN in p0; a state row without a plan"""
    hm = et.hand_made()
    names = list(hm)
    got, want = et.stream_tube(10, 4, np.stack([hm[k] for k in names])), et.numpy_rows(np.stack([hm[k] for k in names]), 4)
    assert max(et.deviations(got, want).values()) <= ATOL
    row = {k: got[i] for i, k in enumerate(names)}
    base = row["base"]
    assert base[TUBE["EX_POS"]] < 0 and base[TUBE["EX_ROT"]] < 0 and base[TUBE["EX_Q"]] < 0 and base[TUBE["EX_DQ"]] < 0
    # 5 cm along bp1: row 39 moves by 0.05, its half width stays
    assert abs(row["pos"][TUBE["L"] + 1] - (base[TUBE["L"] + 1] + 0.05)) <= ATOL and row["pos"][TUBE["W"] + 1] == base[TUBE["W"] + 1]
    assert abs(row["pos"][TUBE["EX_POS"]] - (abs(base[TUBE["L"] + 1] + 0.05) - abs(base[TUBE["W"] + 1]))) <= ATOL and 0.03 < row["pos"][TUBE["EX_POS"]] < 0.05
    assert abs(row["q"][TUBE["EX_Q"]] - (2.1 - np.deg2rad(115.0))) <= 1e-15 and row["q"][TUBE["EX_DQ"]] == base[TUBE["EX_DQ"]]
    assert abs(row["dq"][TUBE["EX_DQ"]] - (1.4 - np.deg2rad(75.0))) <= 1e-15 and row["dq"][TUBE["EX_Q"]] == base[TUBE["EX_Q"]]
    nan = row["nan"]
    assert np.isnan(nan[[TUBE["L"] + 1, TUBE["L"] + 2, TUBE["EX_POS"]]]).all() and np.array_equal(nan[[0, 3, 4, 11, 12, 13, 14, 15]], base[[0, 3, 4, 11, 12, 13, 14, 15]])
    # whole vectors of NaN and of huge numbers: non-finite rows, no crash, the segment in range
    wild = et.stream_tube(10, 4, np.stack([np.full(505, np.nan), np.full(505, 1e300), np.full(505, np.inf)]))
    assert np.isnan(wild[0, :14]).all() and wild[0, TUBE["SEG"]] == 3 and set(wild[:, TUBE["SEG"]]) <= {0.0, 1.0, 2.0, 3.0}
    # state rows: error count N (and a NaN count) -> no plan, an all-NaN row; N - 1 -> the row
    ss = np.zeros((3, bstream.ss_len(10)))
    ss[0, SS["ERRCNT"]], ss[1, SS["ERRCNT"]], ss[2, SS["ERRCNT"]] = 10, 9, np.nan
    out = et.stream_tube(10, 4, np.stack([hm["base"]] * 3), ss)
    assert np.isnan(out[0]).all() and np.isnan(out[2]).all() and np.array_equal(out[1], base)
    # the refusals of the entry
    assert et.stream_tube(10, 4, None, want_rc=True) == 1 and et.stream_tube(10, 4, hm["base"], want_rc=True, B=0) == 1
    assert et.stream_tube(10, 4, hm["base"], want_rc=True) == 0


def test_the_numpy_reduction_handles_every_rule():
    """audit_of on made-up rows: the first of equal maxima, a non-finite excess, the joint bound, rows not run"""
    rows = np.full((5, 16), np.nan)
    for t, (ep, er_, eq, edq) in enumerate([(-1.0, -2.0, -1.0, -1.0), (0.5, -2.0, 2e-9, -1.0), (0.5, np.inf, -1.0, 5e-10), (0.1, 0.3, -1.0, -1.0)]):
        rows[t, 10:14], rows[t, 14] = (ep, er_, eq, edq), 0.0
    a = et.audit_of(rows, 0.2)
    assert a[AUDIT["SAMPLES"]] == 4 and a[AUDIT["MAX_POS"]] == 0.5 and a[AUDIT["TICK_POS"]] == 1 and np.isnan(a[AUDIT["MAX_ROT"]]) and a[AUDIT["TICK_ROT"]] == 2
    assert a[AUDIT["N_POS"]] == 2 and a[AUDIT["N_ROT"]] == 2 and a[AUDIT["N_JOINT"]] == 1 and a[AUDIT["FIRST_OUT"]] == 1 and a[AUDIT["MAX_Q"]] == 2e-9
    # ... and the device text's record over the same rows is the same record
    got = np.zeros(12)
    et.lib().bmpc_emu_stream_audit(4, emu._p(np.ascontiguousarray(rows[:4])), ctypes.c_double(0.2), emu._p(got))
    assert np.array_equal(got, a, equal_nan=True)


@functools.lru_cache(maxsize=None)
def _rollouts():
    """(2, 2), B = 3 on one workgroup, T = 6, the disturbance: the rollout with the audit, the rollout with events without it, and per stream the
    per-tick loop with the tube text on every p -- computed once"""
    opts = er.opts(N)
    _, A0, Tab, _ = er.small_batch(N, S)
    d = er.push(T, 3)
    A, B_ = {k: v.copy() for k, v in A0.items()}, {k: v.copy() for k, v in A0.items()}
    with_audit = er.rollout(N, S, H, Tab.copy(), A, T, entry=2, disturb=d, opts=opts, audit_tol=TOL)
    without = er.rollout(N, S, H, Tab.copy(), B_, T, entry=1, disturb=d, opts=opts)
    loops = []
    for b in range(3):
        Ab = er.unstack(A0, b)
        loops.append(er.contract_loop(N, S, H, Tab[b].copy(), Ab, T, disturb=d[:, b], opts=opts))
    return with_audit, A, without, B_, np.stack([l["tube_hist"] for l in loops], axis=1), A0, Tab, np.stack([l["p_hist"] for l in loops], axis=1)


def test_rollout_audit_equals_the_per_tick_loop_and_the_numpy_reduction():
    r, A, r0, A_plain, loop_rows, _, _, loop_p = _rollouts()
    assert r["ticks_run"].tolist() == [T] * 3
    # numpy on the p the loop packed: the disturbed sample is outside the position tube by more than the tolerance, and the rows are numpy's
    by_numpy = et.numpy_rows(loop_p.reshape(-1, loop_p.shape[-1]), S).reshape(T, 3, -1)
    assert by_numpy[3, 1, TUBE["EX_POS"]] > 1e-3 > TOL and max(et.deviations(loop_rows.reshape(-1, 16), by_numpy.reshape(-1, 16)).values()) <= ATOL
    assert np.array_equal(r["tube_hist"], loop_rows, equal_nan=True)                   # bit for bit
    ex = r["tube_hist"][:, :, TUBE["EX_POS"]]
    assert ex[3, 1] > 1e-3 > TOL and (ex[:3] < 0).all() and (ex[:, [0, 2]] < 0).all()
    want = et.audit_of_batch(r["tube_hist"], TOL)
    assert np.array_equal(r["audit"], want, equal_nan=True)
    a1 = bstream.unpack_audit(r["audit"][1])
    assert a1["first_out"] == 3 and a1["samples"] == T and a1["tick_pos"] == 3 and a1["max_pos"] == ex[3, 1] and a1["n_pos"] >= 1
    assert bstream.unpack_audit(r["audit"][0])["first_out"] is None and bstream.unpack_audit(r["audit"][2])["n_pos"] == 0
    assert r["audit"][:, AUDIT["LEN"] - 1].tolist() == [0.0] * 3


def test_the_audit_changes_nothing_else():
    r, A, r0, A_plain = _rollouts()[:4]
    for k in A:
        assert np.array_equal(A[k], A_plain[k], equal_nan=True), k
    for k in ("hist", "traj_hist", "ticks_run", "replan_info"):
        assert np.array_equal(r[k], r0[k], equal_nan=True), k


def test_either_array_alone_and_neither():
    _, _, r0, A_plain, _, A0, Tab, _ = _rollouts()
    full = _rollouts()[0]
    opts, d = er.opts(N), er.push(T, 3)
    for kw in (dict(audit=False), dict(want_tube=False), dict(audit=False, want_tube=False)):
        A = {k: v.copy() for k, v in A0.items()}
        r = er.rollout(N, S, H, Tab.copy(), A, T, entry=2, disturb=d, opts=opts, audit_tol=TOL, **kw)
        for k in A:
            assert np.array_equal(A[k], A_plain[k], equal_nan=True), (kw, k)
        assert np.array_equal(r["hist"], r0["hist"], equal_nan=True)
        if r["tube_hist"] is not None:
            assert np.array_equal(r["tube_hist"], full["tube_hist"], equal_nan=True)
        if r["audit"] is not None:
            assert np.array_equal(r["audit"], full["audit"], equal_nan=True)


def test_stopped_streams_have_nan_rows_and_their_samples():
    """stream 0 stops at its goal inside the launch, stream 2 is lost on entry"""
    A0, Tab = _rollouts()[5:7]
    A = {k: v.copy() for k, v in A0.items()}
    A["ss"][2, SS["ERRCNT"]] = float(N)
    r = er.rollout(N, S, H, Tab.copy(), A, T, entry=2, opts=er.opts(N), goal_tol=6.9242, audit_tol=TOL)
    run = r["ticks_run"].tolist()
    assert 0 < run[0] < T and run[2] == 0
    for b in range(3):
        assert not np.isnan(r["tube_hist"][:run[b], b]).any() and np.isnan(r["tube_hist"][run[b]:, b]).all()
        assert r["audit"][b, AUDIT["SAMPLES"]] == run[b]
    lost = r["audit"][2]
    assert lost[AUDIT["FIRST_OUT"]] == -1 and lost[AUDIT["TICK_POS"]] == -1 and (lost[[AUDIT["MAX_POS"], AUDIT["MAX_ROT"], AUDIT["MAX_Q"], AUDIT["MAX_DQ"]]] == -np.inf).all()
    assert np.array_equal(r["audit"], et.audit_of_batch(r["tube_hist"], TOL), equal_nan=True)


def test_argument_refusals_mirror_the_entry():
    A0, Tab = _rollouts()[5:7]
    A = {k: v.copy() for k, v in A0.items()}
    call = lambda **kw: er.rollout(N, S, H, Tab.copy(), A, kw.pop("ticks", T), entry=2, opts=er.opts(N), want_rc=True, **kw)
    for kw in (dict(audit_tol=-1e-9), dict(audit_tol=float("nan")), dict(audit_tol=float("inf")), dict(ticks=0), dict(simulate=False), dict(goal_tol=-1.0), dict(update_flags=8),
               dict(replan=np.zeros((3, bstream.replan_len(S, Tab.shape[1])))), dict(audit_tol=-1.0, audit=False, want_tube=False)):
        assert call(**kw) == 1, kw
    for k in A:
        assert np.array_equal(A[k], A0[k], equal_nan=True), k      # nothing ran
